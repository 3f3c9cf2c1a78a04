"""The dispatch sweep on the GPU (tmh_set_dispatch_sweep, BatchedSim.enable_dispatch_sweep; fp64 throughout): K rule
sets per chain in one run, every variant's thirteen columns and state of charge bit for bit dispatch.from_traces of
the traces of separate sims of the same chains (test_gpu_storage.a60_gpu / c60_traces: computed once, shared with
the storage, battery and dispatch tests), never from the kernels under test.  The variants are
dispatch_sweep_util's two sets of K = 5: above the kernels' variants per launch and no multiple of it, so a full
group of launches, a shorter last group and the one-launch rule of the statistics all run."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from dispatch_sweep_util import K, MIN_ROLLED_SHARE, MIN_RULES_SHARE, pair_shares, rolled, rules, rules_equalities
from dispatch_util import NO_LIMIT, identities, soc_changes
from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth
from storage_util import A_BATTERY, modules_params
from test_gpu_registers import C_LEAD, C_START, C_STEPS, C_WINDOWS, _run_windows
from test_gpu_series import _last, _np, _sim
from test_gpu_storage import IV, PREC, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARAMS, SOC0 = rolled()
RULE_PARAMS, RULE_SOC0 = rules()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _enable(sim, n_steps, interval_s, params=PARAMS, soc0=SOC0, **kw):
    """enable_dispatch_sweep with ready parameters and a caller-owned soc (the rolled set's by default)."""
    return sim.enable_dispatch_sweep(n_steps, interval_s, params=_dev(params), soc=_dev(soc0), **kw)


def _want(params, soc0):
    from tmhpvsim_amd import dispatch
    t = a60_gpu()
    got = [dispatch.from_traces(t["pv"], t["meter"], t["cov"], IV, params=params[v], soc0=soc0[v]) for v in range(len(params))]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


@functools.lru_cache(maxsize=None)
def a_want():
    """The expected tables and end states of input A under the rolled set, variant by variant from the storage tests' traces."""
    return _want(PARAMS, SOC0)


def _a_run(params, soc0):
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, A_STEPS, IV, params, soc0)
    k = len(params)
    assert tuple(raw.shape) == (k, 13, 13, A_N) and tuple(sim.soc.shape) == (k, A_N) and sim.soc.dtype == torch.int64
    assert tuple(sim.dispatch_params.shape) == (k, 9, A_N) and sim.dispatch_sweep_raw is raw
    variants_, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), soc=_np(sim.soc), variants=variants_, guards=guards, status=sim.status(),
                watts=sim.dispatch_sweep())


@functools.lru_cache(maxsize=None)
def a_sw():
    """The sweep sim of input A under the rolled set, one tmh_run per window of A_WINDOWS."""
    return _a_run(PARAMS, SOC0)


@functools.lru_cache(maxsize=None)
def a_rules():
    """The same under the rules set."""
    return _a_run(RULE_PARAMS, RULE_SOC0)


def _check_variants(g, want, end, params, soc0):
    """Every variant's thirteen columns and soc bit for bit; columns 0-3 equal across variants; dead chains untouched;
    the cells' identities and the intervals' SoC changes."""
    dead = g["status"] == 1
    assert dead.any()
    for v in range(len(params)):
        for col in range(13):
            np.testing.assert_array_equal(g["raw"][v, :, col], want[v, :, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(g["soc"][v], end[v], err_msg=f"variant {v} soc")
        assert not g["raw"][v][:, :, dead].any() and (g["soc"][v][dead] == soc0[v][dead]).all()
        identities(g["raw"][v], params[v])
        soc_changes(g["raw"][v], soc0[v], g["soc"][v])
        np.testing.assert_array_equal(g["raw"][v, :, :4], g["raw"][0, :, :4])


def test_sweep_equals_the_traces_tables():
    """The main test: every variant's thirteen columns and state of charge bit for bit, over two windows (the second
    off the four-step grid), chains faulted at construction and inside the window, night and day; variant 0 is the
    dispatch kind's own run."""
    from test_gpu_dispatch import a_dp
    from tmhpvsim_amd import _lib, dispatch
    g, t = a_sw(), a60_gpu()
    want, end = a_want()
    a_has_teeth(t["pv"], t["cov"], g["status"])
    live = g["status"] == 0
    shares = pair_shares(want, live, (4,))
    print("column-4 shares", {k: round(s, 4) for k, s in shares.items()})
    assert min(shares.values()) >= MIN_ROLLED_SHARE
    assert g["variants"] == [_lib.OUT_DISPATCH_SWEEP | _lib.OUT_FP64] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    _check_variants(g, want, end, PARAMS, SOC0)
    for v in range(K):
        w = dispatch.to_watts(want[v], IV, n_steps=A_STEPS)
        assert set(g["watts"][v]) == set(w)
        for key in w:
            np.testing.assert_array_equal(g["watts"][v][key], w[key], err_msg=key)
    d = a_dp()                                                             # variant 0: the recipe, the dispatch kind's own run
    np.testing.assert_array_equal(g["raw"][0], d["raw"])
    np.testing.assert_array_equal(g["soc"][0], d["soc"])


def test_one_household_five_rules():
    """The rules set: the recipe's batteries under five (Tc, Td, L).  Variants 0 and 1 differ in the limit alone and are
    equal, exactly, in everything the limit must not touch (a kernel that lets the limit leak into the battery, or
    reads another variant's rows 6-8, fails here); every pair of rules differs for most live chains."""
    from tmhpvsim_amd import _lib
    g = a_rules()
    want, end = _want(RULE_PARAMS, RULE_SOC0)
    live = g["status"] == 0
    assert g["variants"] == [_lib.OUT_DISPATCH_SWEEP | _lib.OUT_FP64] * len(A_WINDOWS)
    _check_variants(g, want, end, RULE_PARAMS, RULE_SOC0)
    shares = pair_shares(g["raw"], live, (4, 5, 10))
    print("columns 4, 5, 10 shares", {k: round(s, 4) for k, s in shares.items()})
    assert min(shares.values()) >= MIN_RULES_SHARE
    share5 = rules_equalities(g["raw"], g["soc"], live)
    print("rules 0 against 1: column 5 differs for", round(share5, 4))
    assert share5 >= 0.9


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
    """Boundaries inside four-second groups (7) and one per 128-s block (128); the origin C_LEAD steps before the run; a
    partial wavefront, more than one workgroup and construction faults; the C levels (thresholds and limits that bind
    just after sunrise) tiled past A_N and rolled."""
    from tmhpvsim_amd import _lib, dispatch
    pv, meter, cov = c60_traces(n)
    par, soc0 = rolled(K, n, "C")
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, C_STEPS + C_LEAD, interval_s, par, soc0, step0=-C_LEAD)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_DISPATCH_SWEEP | _lib.OUT_FP64
    torch.cuda.synchronize()
    got, soc = _np(raw), _np(sim.soc)
    assert got.shape == (K, -(-(C_STEPS + C_LEAD) // interval_s), 13, n)
    if n > 1000:
        assert (cov[0] == 255).any()                                       # construction faults
    curtailed = 0
    for v in range(K):
        want, end = dispatch.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, params=par[v], soc0=soc0[v])
        for col in range(13):
            np.testing.assert_array_equal(got[v, :, col], want[:, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(soc[v], end, err_msg=f"variant {v}")
        identities(got[v], par[v])
        soc_changes(got[v], soc0[v], soc[v])
        assert int(want[:, 6].sum()) > 0 and int(want[:, 7].sum()) > 0
        curtailed += int(want[:, 10].sum())
    assert curtailed > 0 and (got[0, :, 4:] != got[K - 1, :, 4:]).any()


def test_variant_counts():
    """K = 1 is enable_dispatch bit for bit (a group of one: the dispatch kind's own kernels) and the first slice of
    the K = 5 sweep; sweeps over the first two and the first three variants are the K = 5 sweep's slices.  Whichever
    count of variants per launch between 2 and 4 is built, these run a full group, a group of one and, above 2, a
    short group inside the sweep's kernels."""
    from test_gpu_dispatch import a_dp
    from tmhpvsim_amd import _lib
    g, d = a_sw(), a_dp()
    for k in (1, 2, 3):
        sim = _sim(A_N, A_START, **_kw60())
        r = _enable(sim, A_STEPS, IV, PARAMS[:k], SOC0[:k])
        _run_windows(sim, A_WINDOWS)
        assert _last(sim) == _lib.OUT_DISPATCH_SWEEP | _lib.OUT_FP64 and tuple(r.shape) == (k, 13, 13, A_N)
        np.testing.assert_array_equal(_np(r), g["raw"][:k], err_msg=f"K = {k}")
        np.testing.assert_array_equal(_np(sim.soc), g["soc"][:k], err_msg=f"K = {k}")
        if k == 1:
            np.testing.assert_array_equal(_np(r)[0], d["raw"])
            np.testing.assert_array_equal(_np(sim.soc)[0], d["soc"])
    assert (g["raw"][1, :, 4:] != g["raw"][0, :, 4:]).any() and (g["raw"][2, :, 4:] != g["raw"][1, :, 4:]).any()


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_statistics_unperturbed_by_the_sweep(spec):
    """Statistics beside the sweep are the statistics-only run's, bit for bit: of the groups' replay launches exactly
    one accumulates them (two would double the histogram and the energies), the map passes none."""
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
    assert _last(both) == _lib.OUT_DISPATCH_SWEEP | _lib.OUT_FP64 and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and torch.equal(both.soc, alone.soc) and int(ra[0, :, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[0, :, 2].sum()) == int(ra[K - 1, :, 2].sum())
    for v in range(K):
        assert int(ra[v, :, 6].sum()) > 0 and int(ra[v, :, 7].sum()) > 0 and int(ra[v, :, 9].sum()) > 0
        identities(_np(ra[v]), par[v])


def test_two_batches_fill_one_table():
    """Chains [5000, 5500) and [5500, 6000) as two sims writing column slices of one [K, 13, 13, 1000] table, reading
    slices of one [K, 9, 1000] params tensor and carrying slices of one [K, 1000] soc."""
    want, end = a_want()
    big = torch.zeros(K, 13, 13, A_N, dtype=torch.int64, device="cuda:0")
    params, soc = _dev(PARAMS), _dev(SOC0)
    for a, b in ((0, 500), (500, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        view = big[:, :, :, a:b]
        got = s.enable_dispatch_sweep(A_STEPS, IV, buffer=view, soc=soc[:, a:b], params=params[:, :, a:b])
        assert got is view and s._dispatch_sweep.ld == A_N and s.soc.data_ptr() == soc[:, a:b].data_ptr()
        assert s.dispatch_params.data_ptr() == params[:, :, a:b].data_ptr()
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), want)
    np.testing.assert_array_equal(_np(soc), end)
    np.testing.assert_array_equal(_np(params), PARAMS)                                     # read only
    with pytest.raises(ValueError, match="strides"):
        s.enable_dispatch_sweep(A_STEPS, IV, buffer=big[:, :, :, :2 * s.n:2], params=params[:, :, 500:], soc=soc[:, 500:])
    with pytest.raises(ValueError, match="dispatch sweep buffer"):
        s.enable_dispatch_sweep(A_STEPS, IV, buffer=torch.zeros(K, 13, 10, s.n, dtype=torch.int64, device="cuda:0"),
                                params=params[:, :, 500:], soc=soc[:, 500:])
    with pytest.raises(ValueError, match="same width"):                                    # params of another width than the table
        s.enable_dispatch_sweep(A_STEPS, IV, params=params[:, :, 500:])
    with pytest.raises(ValueError, match="params"):
        s.enable_dispatch_sweep(A_STEPS, IV, buffer=big[:, :, :, 500:], params=params[:, :, :2 * s.n:2], soc=soc[:, 500:])
    with pytest.raises(ValueError, match="params"):                                        # the battery sweep's six rows only
        s.enable_dispatch_sweep(A_STEPS, IV, buffer=big[:, :, :, 500:], params=params[:, :6, 500:], soc=soc[:, 500:])
    with pytest.raises(ValueError, match="soc"):
        s.enable_dispatch_sweep(A_STEPS, IV, buffer=big[:, :, :, 500:], params=params[:, :, 500:], soc=soc[:, :2 * s.n:2])
    s.enable_dispatch_sweep(None)
    assert s.soc is None and s.dispatch_sweep_raw is None and s.dispatch_params is None


def test_reductions_to_the_battery_kind_and_the_battery_sweep():
    """Tc = Td = 0 and no limit: the rules set's variant 0 is the battery kind's own run of the recipe's batteries in
    columns 0-9 and soc (test_gpu_battery.a_bt), column 10 is 0; the whole sweep with those rules over sweep_util's
    batteries is enable_battery_sweep's run (test_gpu_battery_sweep.a_sw) in columns 0-9 and soc."""
    import sweep_util
    from test_gpu_battery import a_bt
    from test_gpu_battery_sweep import a_sw as battery_a_sw
    from tmhpvsim_amd import _lib
    g, b = a_rules(), a_bt()
    np.testing.assert_array_equal(g["raw"][0][:, :10], b["raw"])
    np.testing.assert_array_equal(g["soc"][0], b["soc"])
    assert not g["raw"][0][:, 10].any() and int(b["raw"][:, 6].sum()) > 0
    bpar, bsoc = sweep_util.variants()
    greedy = np.zeros((sweep_util.K, 9, A_N), dtype=np.int64)
    greedy[:, :6], greedy[:, 8] = bpar, NO_LIMIT
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV, greedy, bsoc)
    _run_windows(sim, A_WINDOWS)
    assert _last(sim) == _lib.OUT_DISPATCH_SWEEP | _lib.OUT_FP64
    bs = battery_a_sw()
    got = _np(raw)
    np.testing.assert_array_equal(got[:, :, :10], bs["raw"])
    np.testing.assert_array_equal(_np(sim.soc), bs["soc"])
    assert not got[:, :, 10].any() and int((got[:, :, 12] >> 32).max()) > 0


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "dispatch sweep" before anything is launched: the
    chains' state and the batteries' stay as they were and the tables all zeros; what was enabled before still works."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams, site_grid
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, soc0 = PARAMS[:, :, :n], SOC0[:, :n]
    BAT = dict(capacity_wh=0.5, charge_w=1000.0, discharge_w=3000.0, charge_eff=0.95, discharge_eff=0.9, standby_w=1.0,
               soc0_wh=0.25)
    DSP = dict(BAT, charge_above_w=250.0, discharge_above_w=2000.0, feed_in_limit_w=500.0)
    SW = dict(BAT, capacity_wh=[0.5, 0.25, 0.75], charge_above_w=[0.0, 250.0, 500.0], discharge_above_w=2000.0,
              feed_in_limit_w=[None, 500.0, 250.0])

    def refused(sim, match, step0=0, k=100, trace=None, inj=None, raw=None):
        before, soc = sim.state.clone(), sim.soc.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        ij = C.byref(inj) if inj is not None else None
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg and "dispatch sweep" in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if sim.path == "time_parallel" and trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and torch.equal(soc, sim.soc)
        assert not bool((sim.dispatch_sweep_raw if raw is None else raw).any())

    def desc(sim, **kw):
        """The sim's tmh_dispatch_sweep with fields replaced."""
        d = sim._dsweep_desc
        f = dict(table=d.table, soc=d.soc, work=d.work, work_bytes=d.work_bytes, params=d.params, n_variants=d.n_variants)
        return _lib.DispatchSweep(**{**f, **kw})

    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, soc0)
    out = torch.zeros(100, n, dtype=torch.float64, device="cuda:0")
    refused(sim, "dispatch sweep tables are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # the sweep, then a fleet series
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    sim.enable_dispatch_sweep(None)
    sim.enable_series(500)                                                 # a fleet series, then the sweep
    with pytest.raises(ValueError, match="fleet series"):
        _enable(sim, 500, 60, par, soc0)
    sim.run(10, trace=())                                                  # the series still works
    torch.cuda.synchronize()
    assert int(sim.series_raw[0, :10, 2].sum()) > 0
    sim.enable_series(None)
    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, soc0)
    refused(sim, "outside the dispatch sweep", step0=0, k=501)             # past the end
    refused(sim, "outside the dispatch sweep", step0=450, k=100)
    _enable(sim, 500, 60, par, soc0, step0=10)
    refused(sim, "outside the dispatch sweep", step0=0, k=100)             # before the origin
    buf = _enable(sim, 500, 60, par, soc0)
    _lib.check(L.tmh_set_dispatch_sweep(sim._eng, C.byref(desc(sim, table=_lib.Intervals(buf.data_ptr(), 0, 500, 60, n - 1)))))
    refused(sim, "dispatch sweep tables ld")                               # ld too small
    _lib.check(L.tmh_set_dispatch_sweep(sim._eng, C.byref(desc(sim, work_bytes=L.tmh_battery_sweep_work_bytes(n, 100, K) - 8))))
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
                     (dict(params=None), b"params"), (dict(params=sim.dispatch_params.data_ptr() + 4), b"params")):
        assert L.tmh_set_dispatch_sweep(sim._eng, C.byref(desc(sim, **kw))) == -1 and word in L.tmh_last_error()
        assert b"dispatch sweep" in L.tmh_last_error()                     # the setter refuses a bad struct
    # the sweep with another table kind on one engine -- the battery sweep and dispatch themselves included -- in either order
    _enable(sim, 500, 60, par, soc0)
    for kind, cols, word in (("intervals", 4, "the dispatch sweep and interval metering"),
                             ("registers", 6, "the dispatch sweep and the import / export registers"),
                             ("demand", 8, "the dispatch sweep and the demand registers"),
                             ("storage", 9, "the dispatch sweep and battery storage"),
                             ("battery", 10, "the dispatch sweep and the battery kind"),
                             ("battery_sweep", 10, "the dispatch sweep and the battery sweep"),
                             ("dispatch", 13, "the dispatch sweep and battery dispatch")):
        other = torch.zeros(9, cols, n, dtype=torch.int64, device="cuda:0")
        tbl = _lib.Intervals(other.data_ptr(), 0, 500, 60, n)
        d = sim._dsweep_desc
        arg = (_lib.Storage(tbl, d.soc, d.work, d.work_bytes, 100, 5, 5) if kind == "storage"
               else _lib.Battery(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "battery"
               else _lib.BatterySweep(tbl, d.soc, d.work, d.work_bytes, d.params, 1) if kind == "battery_sweep"
               else _lib.Dispatch(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "dispatch" else tbl)
        setter = getattr(L, "tmh_set_" + kind)
        _lib.check(setter(sim._eng, C.byref(arg)))
        refused(sim, word)
        _lib.check(L.tmh_set_dispatch_sweep(sim._eng, None))
        _lib.check(L.tmh_set_dispatch_sweep(sim._eng, C.byref(sim._dsweep_desc)))   # (now the sweep after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
        extra = A_BATTERY if kind == "storage" else BAT if kind in ("battery", "battery_sweep") else DSP if kind == "dispatch" else {}
        with pytest.raises(ValueError, match="the dispatch sweep"):
            getattr(sim, "enable_" + kind)(500, 60, **extra)
        o = _sim(64, start, prec=PREC, horizon=1000)
        oraw = getattr(o, "enable_" + kind)(500, 60, **extra)
        with pytest.raises(ValueError, match="one table output per sim"):
            o.enable_dispatch_sweep(500, 60, **SW)
        o.run(60, trace=())                                                # the table enabled before still works
        torch.cuda.synchronize()
        first = oraw[0, 0, 2] if kind == "battery_sweep" else oraw[0, 2]
        assert int(first.sum()) > 0 and o.dispatch_sweep_raw is None
    # the battery fleet series: the battery kind's own output, in either order
    fl = torch.zeros(1, 500, 8, dtype=torch.int64, device="cuda:0")
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(_lib.Series(fl.data_ptr(), 0, 500, 0, 1, 0))))
    refused(sim, "battery fleet series")
    _lib.check(L.tmh_set_dispatch_sweep(sim._eng, None))
    _lib.check(L.tmh_set_dispatch_sweep(sim._eng, C.byref(sim._dsweep_desc)))
    refused(sim, "battery fleet series")
    assert not bool(fl.any())
    _lib.check(L.tmh_set_battery_fleet(sim._eng, None))
    with pytest.raises(ValueError, match="enable_battery first"):
        sim.enable_battery_fleet(500)
    o = _sim(64, start, prec=PREC, horizon=1000)
    o.enable_battery(500, 60, **A_BATTERY)
    o.enable_battery_fleet(500)
    with pytest.raises(ValueError, match="one table output per sim|battery fleet series"):
        o.enable_dispatch_sweep(500, 60, **SW)
    o.run(60, trace=())
    torch.cuda.synchronize()
    assert int(o.battery_fleet_raw[0, :60, 2].sum()) > 0 and int(o.battery_raw[0, 2].sum()) > 0
    # per-chain sites
    ss = _sim(64, start, prec=PREC, horizon=1000, sites=site_grid(8, 8))
    with pytest.raises(ValueError, match="per-chain sites"):
        ss.enable_dispatch_sweep(500, 60, **SW)
    sraw = torch.zeros(K, 9, 13, 64, dtype=torch.int64, device="cuda:0")
    ssoc, spar = _dev(SOC0[:, :64]), _dev(PARAMS[:, :, :64])
    swork = torch.empty(L.tmh_battery_sweep_work_bytes(64, 500, K), dtype=torch.uint8, device="cuda:0")
    sdesc = _lib.DispatchSweep(_lib.Intervals(sraw.data_ptr(), 0, 500, 60, 64), ssoc.data_ptr(), swork.data_ptr(), swork.numel(),
                               spar.data_ptr(), K)
    _lib.check(L.tmh_set_dispatch_sweep(ss._eng, C.byref(sdesc)))
    ss.soc = ssoc
    refused(ss, "per-chain sites", raw=sraw)
    _lib.check(L.tmh_set_dispatch_sweep(ss._eng, None))
    seq = _sim(64, start, prec=PREC, horizon=1000, kernel_path="sequential")   # the sequential path
    seq.enable_dispatch_sweep(500, 60, **SW)
    refused(seq, "dispatch sweep tables need the time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), precision=PREC, device="cuda:0",
                      injected=inj, horizon=1000)
    isim.enable_dispatch_sweep(500, 60, **SW)
    refused(isim, "time-parallel", inj=isim._us)
    mp = ModelParams()
    mp.inverter = dict(mp.inverter, Paco=float(L.tmh_series_max_w()))      # Paco >= TMH_SERIES_MAX_W
    big = _sim(64, start, prec=PREC, mp=mp, horizon=1000)
    big.enable_dispatch_sweep(500, 60, **SW)
    refused(big, "TMH_SERIES_MAX_W")
    # fp32 engines: refused at the setter and at enable_dispatch_sweep
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    with pytest.raises(ValueError, match="fp64"):
        f32.enable_dispatch_sweep(500, 60, **SW)
    assert L.tmh_set_dispatch_sweep(f32._eng, C.byref(sim._dsweep_desc)) == -1
    assert b"fp64" in L.tmh_last_error() and b"dispatch sweep" in L.tmh_last_error()
    # the Python layer refuses values outside their ranges before upload, a soc0 outside [0, C], lists of two lengths
    for bad in (dict(capacity_wh=1e9), dict(charge_w=-1.0), dict(charge_eff=0.4), dict(discharge_eff=[1.1, 1.0, 1.0]),
                dict(standby_w=-1.0), dict(soc0_wh=0.6), dict(soc0_wh=-0.1), dict(charge_w=[1.0, 2.0]),
                dict(capacity_wh=[0.5] * 17), dict(n_variants=4), dict(charge_above_w=[0.0, -1.0, 0.0]),
                dict(discharge_above_w=40000.0), dict(feed_in_limit_w=[None, -1.0, None]),
                dict(feed_in_limit_w=float("nan")), dict(feed_in_limit_w=[None, 1.0])):
        with pytest.raises(ValueError):
            sim.enable_dispatch_sweep(500, 60, **{**SW, **bad})
    worse = par.copy()
    worse[2, 8, 5] = (1 << 27) + 1
    with pytest.raises(ValueError, match="feed_in_limit"):
        sim.enable_dispatch_sweep(500, 60, params=_dev(worse))
    with pytest.raises(ValueError, match="required"):
        sim.enable_dispatch_sweep(500, 60)

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_dispatch_sweep(500, 60, **SW)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the dispatch sweep"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.dispatch_sweep_raw.any())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw, hostpar = _np(sim.dispatch_sweep_raw), _np(sim.dispatch_params)
    assert raw.shape == (3, 9, 13, n) and (hostpar[0, 8] == NO_LIMIT).all() and (hostpar[2, 8] == 250 << 12).all()
    for v in range(3):
        assert int(raw[v, :2, 2].sum()) > 0 and not raw[v, 2:].any()
        identities(raw[v], hostpar[v])
    assert L.tmh_set_dispatch_sweep(sim._eng, None) == 0                   # NULL: off


def test_dispatch_sweep_cli(tmp_path):
    """A CSV row per variant (its parameters, the fleet's totals and ratios) and the .npz's tables, against
    sweep_summary of the tables that sweep_from_traces gives for the traces of a separate sim."""
    from click.testing import CliRunner
    from tmhpvsim_amd import dispatch
    from tmhpvsim_amd.cli import DISPATCH_SWEEP_OPTIONS, DISPATCH_SWEEP_RATIOS, DISPATCH_SWEEP_TOTALS, main
    from tmhpvsim_amd.params import ModelParams
    f, z = tmp_path / "ds.csv", tmp_path / "ds.npz"
    n, steps, iv = 64, 1800, 600
    caps = [0.05, 0.0, 0.02, 0.05, 0.1]
    r = CliRunner().invoke(main, ["dispatch-sweep", str(f), "--batch", str(n), "--seconds", str(steps), "--interval", str(iv),
                                  "--no-realtime", "--capacity-wh", ",".join(map(str, caps)), "--charge-w", "1000",
                                  "--discharge-w", "3000,1500,3000,3000,50", "--charge-eff", "0.95", "--discharge-eff",
                                  "0.9,1.0,1.0,0.9,0.9", "--standby-w", "2", "--soc0-wh", "0.02,0,0.01,0,0.1",
                                  "--charge-above-w", "0,0,20,20,40", "--discharge-above-w", "100",
                                  "--feed-in-limit-w", "none,10,10,none,60", "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    opts = dict(capacity_wh=caps, charge_w=[1000.0] * 5, discharge_w=[3000.0, 1500.0, 3000.0, 3000.0, 50.0],
                charge_eff=[0.95] * 5, discharge_eff=[0.9, 1.0, 1.0, 0.9, 0.9], standby_w=[2.0] * 5,
                soc0_wh=[0.02, 0.0, 0.01, 0.0, 0.1], charge_above_w=[0.0, 0.0, 20.0, 20.0, 40.0],
                discharge_above_w=[100.0] * 5, feed_in_limit_w=[None, 10.0, 10.0, None, 60.0])
    par = dispatch.quantize_sweep_params(*(opts[o] for o in DISPATCH_SWEEP_OPTIONS if o != "soc0_wh"), n=n)
    soc0 = dispatch.quantize_sweep_soc(opts["soc0_wh"], par)
    tr = _sim(n, "2019-09-06T12:00:00", prec=PREC, mp=ModelParams(seed=0x5EED), horizon=steps)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    want, end = dispatch.sweep_from_traces(out["pv"], out["meter"], out["covered"], iv, params=par, soc0=soc0)
    saved = np.load(z)
    assert saved["raw"].shape == (5, 3, 13, n) and int(saved["interval_s"]) == iv
    np.testing.assert_array_equal(saved["raw"], want)
    np.testing.assert_array_equal(saved["soc"], end)
    np.testing.assert_array_equal(saved["params"], par)
    fleet = dispatch.sweep_summary(want, iv, par, fleet=True)
    rows = list(csv.reader(open(f)))
    assert rows[0] == (["variant"] + list(DISPATCH_SWEEP_OPTIONS) + [h for h, _ in DISPATCH_SWEEP_TOTALS]
                       + list(DISPATCH_SWEEP_RATIOS)) and len(rows) == 1 + 5
    no = len(DISPATCH_SWEEP_OPTIONS)
    for v, row in enumerate(rows[1:]):
        assert int(row[0]) == v
        assert [None if x == "none" else float(x) for x in row[1:1 + no]] == [opts[o][v] for o in DISPATCH_SWEEP_OPTIONS]
        got = [float(x) for x in row[1 + no:]]
        exp = [float(fleet[key][v]) for _, key in DISPATCH_SWEEP_TOTALS] + [float(fleet[key][v]) for key in DISPATCH_SWEEP_RATIOS]
        assert all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(got, exp)), (v, got, exp)
    head = rows[0]
    cur, pex = head.index("curtailed_wh"), head.index("peak_export_w")
    assert float(rows[1][cur]) == 0 and float(rows[2][cur]) > 0 and float(rows[2][pex]) == 10.0   # no limit; a limit that binds
    assert float(rows[1][1 + no]) != float(rows[5][1 + no])                  # another rule and battery, another import
