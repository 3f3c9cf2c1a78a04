"""The schedule sweep on the GPU (tmh_set_schedule_sweep, BatchedSim.enable_schedule_sweep; fp64 throughout): K
(battery, rule sets, rule array) variants per chain in one run, every variant's thirteen columns and state of charge
bit for bit schedule.from_traces of the traces of separate sims of the same chains (test_gpu_storage.a60_gpu /
c60_traces: computed once, shared with the storage, battery, dispatch and schedule tests) or the schedule kind's and
the dispatch kind's own kernels, never the kernels under test.  The variants are schedule_sweep_util's two sets of
K = 5: above the kernels' variants per launch and no multiple of it, so a full group of launches, a shorter last
group or a group of one, and the one-launch rule of the statistics all run."""
import ctypes as C
import functools

import numpy as np
import pytest

from dispatch_util import identities, soc_changes
from schedule_sweep_util import (K, MIN_ROLLED_SHARE, MIN_TARIFFS_SHARE, MIN_TARIFFS_SHARE4, limit_params, pair_shares, rolled,
                                 tariffs)
from schedule_util import A_RULES, R, recipe, tiled
from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth
from storage_util import A_BATTERY, modules_params
from test_gpu_registers import C_LEAD, C_START, C_STEPS, C_WINDOWS, _run_windows
from test_gpu_series import _last, _np, _sim
from test_gpu_storage import IV, PREC, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARAMS, ARRAYS, SOC0 = rolled()
T_PARAMS, T_ARRAYS, T_SOC0 = tariffs()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _enable(sim, n_steps, interval_s, params=PARAMS, arrays=ARRAYS, soc0=SOC0, **kw):
    """enable_schedule_sweep with ready parameters, the variants' arrays and a caller-owned soc (the rolled set's by default)."""
    return sim.enable_schedule_sweep(n_steps, interval_s, params=_dev(params), rule_of_interval=arrays, soc=_dev(soc0), **kw)


def _want(params, arrays, soc0):
    from tmhpvsim_amd import schedule
    t = a60_gpu()
    got = [schedule.from_traces(t["pv"], t["meter"], t["cov"], IV, params=params[v], rule_of_interval=arrays[v], soc0=soc0[v])
           for v in range(len(params))]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


@functools.lru_cache(maxsize=None)
def a_want():
    """The expected tables and end states of input A under the rolled set, variant by variant from the storage tests' traces."""
    return _want(PARAMS, ARRAYS, SOC0)


def _a_run(params, arrays, soc0):
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, A_STEPS, IV, params, arrays, soc0)
    k = len(params)
    assert tuple(raw.shape) == (k, 13, 13, A_N) and tuple(sim.soc.shape) == (k, A_N) and sim.soc.dtype == torch.int64
    assert tuple(sim.schedule_sweep_params.shape) == (k, 6 + 4 * R, A_N) and sim.schedule_sweep_raw is raw
    assert sim.schedule_sweep_rules.dtype == torch.uint8 and np.array_equal(_np(sim.schedule_sweep_rules), arrays)
    variants_, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), soc=_np(sim.soc), variants=variants_, guards=guards, status=sim.status(), summary=sim.schedule_sweep())


@functools.lru_cache(maxsize=None)
def a_sw():
    """The sweep sim of input A under the rolled set, one tmh_run per window of A_WINDOWS."""
    return _a_run(PARAMS, ARRAYS, SOC0)


def _check_variants(g, want, end, params, arrays, soc0):
    """Every variant's thirteen columns and soc bit for bit; columns 0-3 equal across variants; dead chains untouched;
    the cells' identities under the limit in force and the intervals' SoC changes."""
    dead = g["status"] == 1
    assert dead.any()
    for v in range(len(params)):
        for col in range(13):
            np.testing.assert_array_equal(g["raw"][v, :, col], want[v, :, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(g["soc"][v], end[v], err_msg=f"variant {v} soc")
        assert not g["raw"][v][:, :, dead].any() and (g["soc"][v][dead] == soc0[v][dead]).all()
        identities(g["raw"][v], limit_params(params[v], arrays[v]))
        soc_changes(g["raw"][v], soc0[v], g["soc"][v])
        np.testing.assert_array_equal(g["raw"][v, :, :4], g["raw"][0, :, :4])


def test_rolled_sweep_equals_the_traces_tables():
    """The main test: every variant's thirteen columns and state of charge bit for bit, over two windows (the second
    off the four-step grid), chains faulted at construction and inside the window, night and day, grid charging and
    hold intervals under five shifted arrays; variant 0 is the schedule kind's own run."""
    from test_gpu_schedule import a_sc
    from tmhpvsim_amd import _lib, schedule
    g, t = a_sw(), a60_gpu()
    want, end = a_want()
    a_has_teeth(t["pv"], t["cov"], g["status"])
    live = g["status"] == 0
    shares = pair_shares(want, live, (4,))
    print("column-4 shares", {k: round(s, 4) for k, s in shares.items()})
    assert min(shares.values()) >= MIN_ROLLED_SHARE
    assert g["variants"] == [_lib.OUT_SCHEDULE_SWEEP | _lib.OUT_FP64] * len(A_WINDOWS) == [96] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    _check_variants(g, want, end, PARAMS, ARRAYS, SOC0)
    s = schedule.sweep_summary(want, IV, PARAMS)
    assert set(g["summary"]) == set(s)
    for key in s:
        np.testing.assert_array_equal(g["summary"][key], s[key], err_msg=key)
    d = a_sc()                                                             # variant 0: the recipe, the schedule kind's own run
    np.testing.assert_array_equal(g["raw"][0], d["raw"])
    np.testing.assert_array_equal(g["soc"][0], d["soc"])


def test_one_household_five_tariffs():
    """The tariffs set: the recipe's households under five arrays, nothing else differing.  A kernel that reads another
    variant's array row fails here, in the battery's columns and nowhere in columns 0-3; variant 1 (rule 0 throughout)
    is the dispatch kind's own run under rule 0."""
    from test_gpu_schedule import a_dispatch_rule0
    from tmhpvsim_amd import _lib
    g = _a_run(T_PARAMS, T_ARRAYS, T_SOC0)
    want, end = _want(T_PARAMS, T_ARRAYS, T_SOC0)
    live = g["status"] == 0
    assert g["variants"] == [_lib.OUT_SCHEDULE_SWEEP | _lib.OUT_FP64] * len(A_WINDOWS)
    _check_variants(g, want, end, T_PARAMS, T_ARRAYS, T_SOC0)
    s4, s = pair_shares(g["raw"], live, (4,)), pair_shares(g["raw"], live, (4, 5, 10))
    print("column 4 shares", {k: round(x, 4) for k, x in s4.items()}, "columns 4, 5, 10", {k: round(x, 4) for k, x in s.items()})
    assert min(s4.values()) >= MIN_TARIFFS_SHARE4 and min(s.values()) >= MIN_TARIFFS_SHARE
    dwant, dend = a_dispatch_rule0()
    np.testing.assert_array_equal(g["raw"][1], dwant)
    np.testing.assert_array_equal(g["soc"][1], dend)
    assert not g["raw"][3, :, 6].any() and not g["raw"][3, :, 7].any()      # hold throughout


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
    """Rule changes inside four-second groups (7) and one per 128-s block, off the block grid (128); the origin C_LEAD
    steps before the run; a partial wavefront, more than one workgroup and construction faults; the C recipe tiled past
    A_N and rolled, each variant under its own rolled array.  Both passes must take each second's rule of each variant
    from the second's own interval."""
    from tmhpvsim_amd import _lib, schedule
    pv, meter, cov = c60_traces(n)
    n_iv = -(-(C_STEPS + C_LEAD) // interval_s)
    par, arr, soc0 = rolled(K, n, "C", n_iv)
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, C_STEPS + C_LEAD, interval_s, par, arr, soc0, step0=-C_LEAD)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_SCHEDULE_SWEEP | _lib.OUT_FP64
    torch.cuda.synchronize()
    got, soc = _np(raw), _np(sim.soc)
    assert got.shape == (K, n_iv, 13, n)
    if n > 1000:
        assert (cov[0] == 255).any()                                       # construction faults
    for v in range(K):
        want, end = schedule.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, params=par[v], rule_of_interval=arr[v],
                                         soc0=soc0[v])
        for col in range(13):
            np.testing.assert_array_equal(got[v, :, col], want[:, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(soc[v], end, err_msg=f"variant {v}")
        identities(got[v], limit_params(par[v], arr[v]))
        soc_changes(got[v], soc0[v], soc[v])
        assert int(want[:, 6].sum()) > 0
    assert (got[0, :, 4:] != got[K - 1, :, 4:]).any()


def test_variant_counts():
    """K = 1 is enable_schedule bit for bit (a group of one: the schedule kind's own kernels) and the first slice of
    the K = 5 sweep; sweeps over the first two and the first three variants are the K = 5 sweep's slices.  Whichever
    count of variants per launch between 2 and 4 is built, these run a full group, a group of one and, above 2, a
    short group inside the sweep's kernels."""
    from test_gpu_schedule import a_sc
    from tmhpvsim_amd import _lib
    g, d = a_sw(), a_sc()
    for k in (1, 2, 3):
        sim = _sim(A_N, A_START, **_kw60())
        r = _enable(sim, A_STEPS, IV, PARAMS[:k], ARRAYS[:k], SOC0[:k])
        _run_windows(sim, A_WINDOWS)
        assert _last(sim) == _lib.OUT_SCHEDULE_SWEEP | _lib.OUT_FP64 and tuple(r.shape) == (k, 13, 13, A_N)
        np.testing.assert_array_equal(_np(r), g["raw"][:k], err_msg=f"K = {k}")
        np.testing.assert_array_equal(_np(sim.soc), g["soc"][:k], err_msg=f"K = {k}")
        if k == 1:
            np.testing.assert_array_equal(_np(r)[0], d["raw"])
            np.testing.assert_array_equal(_np(sim.soc)[0], d["soc"])
    assert (g["raw"][1, :, 4:] != g["raw"][0, :, 4:]).any() and (g["raw"][2, :, 4:] != g["raw"][1, :, 4:]).any()


def test_range_end_sixteen_variants_eight_rules():
    """K = 16 with R = 8 on 64 chains x 701 s: variant v's rules are the C recipe's four repeated twice with the
    grid-charge powers scaled by v, its array (k + v) % 8; against sixteen calls of schedule.from_traces."""
    from tmhpvsim_amd import _lib, schedule
    n, interval_s, k16 = 64, 60, 16
    pv, meter, cov = c60_traces(n)
    n_iv = -(-(C_STEPS + C_LEAD) // interval_s)
    base, soc1 = tiled(n, "C")
    par = np.stack([np.vstack([base[:6], base[6:], base[6:]]) for _ in range(k16)]).astype(np.int64)
    for v in range(k16):
        par[v, 9::4] = np.minimum(par[v, 9::4] * v, 1 << 27)
    arr = ((np.arange(n_iv)[None, :] + np.arange(k16)[:, None]) % 8).astype(np.uint8)
    soc0 = np.stack([soc1] * k16).astype(np.int64)
    schedule.check_sweep_params(par, n_rules=8)
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, C_STEPS + C_LEAD, interval_s, par, arr, soc0, step0=-C_LEAD, n_rules=8, n_variants=k16)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_SCHEDULE_SWEEP | _lib.OUT_FP64
    torch.cuda.synchronize()
    got, soc = _np(raw), _np(sim.soc)
    assert got.shape == (k16, n_iv, 13, n)
    for v in range(k16):
        want, end = schedule.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, params=par[v], rule_of_interval=arr[v],
                                         soc0=soc0[v])
        np.testing.assert_array_equal(got[v], want, err_msg=f"variant {v}")
        np.testing.assert_array_equal(soc[v], end, err_msg=f"variant {v}")
    assert (got[15, :, 4:] != got[14, :, 4:]).any() and (got[1, :, 4:] != got[0, :, 4:]).any()


def test_shared_array_and_equal_params():
    """A broadcast [n_intervals] array with equal params in every variant: K equal tables, each the schedule's."""
    from test_gpu_schedule import a_sc
    d = a_sc()
    p0, s0 = recipe()
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV, np.stack([p0] * 3), A_RULES, np.stack([s0] * 3))
    assert tuple(sim.schedule_sweep_rules.shape) == (3, 13)
    _run_windows(sim, A_WINDOWS)
    got, soc = _np(raw), _np(sim.soc)
    for v in range(3):
        np.testing.assert_array_equal(got[v], d["raw"], err_msg=f"variant {v}")
        np.testing.assert_array_equal(soc[v], d["soc"], err_msg=f"variant {v}")


def test_two_batches_fill_one_table():
    """Chains [5000, 5500) and [5500, 6000) as two sims writing column slices of one [K, 13, 13, 1000] table, reading
    slices of one [K, 22, 1000] params tensor and carrying slices of one [K, 1000] soc."""
    want, end = a_want()
    big = torch.zeros(K, 13, 13, A_N, dtype=torch.int64, device="cuda:0")
    params, soc = _dev(PARAMS), _dev(SOC0)
    for a, b in ((0, 500), (500, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        view = big[:, :, :, a:b]
        got = s.enable_schedule_sweep(A_STEPS, IV, buffer=view, soc=soc[:, a:b], params=params[:, :, a:b], rule_of_interval=ARRAYS)
        assert got is view and s._schedule_sweep.ld == A_N and s.soc.data_ptr() == soc[:, a:b].data_ptr()
        assert s.schedule_sweep_params.data_ptr() == params[:, :, a:b].data_ptr()
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), want)
    np.testing.assert_array_equal(_np(soc), end)
    np.testing.assert_array_equal(_np(params), PARAMS)                                     # read only
    with pytest.raises(ValueError, match="strides"):
        s.enable_schedule_sweep(A_STEPS, IV, buffer=big[:, :, :, :2 * s.n:2], params=params[:, :, 500:], soc=soc[:, 500:],
                                rule_of_interval=ARRAYS)
    with pytest.raises(ValueError, match="same width"):                                    # params of another width than the table
        s.enable_schedule_sweep(A_STEPS, IV, params=params[:, :, 500:], rule_of_interval=ARRAYS)
    s.enable_schedule_sweep(None)
    assert s.soc is None and s.schedule_sweep_raw is None and s.schedule_sweep_params is None and s.schedule_sweep_rules is None


def test_statistics_unperturbed_by_the_sweep():
    """Statistics beside the sweep are the statistics-only run's, bit for bit: of the groups' replay launches exactly
    one accumulates them, the map passes none."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw60(steps)
    par, arr, soc0 = PARAMS[:, :, :n], ARRAYS[:, :3], SOC0[:, :n]
    both, stats, alone = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats(**HISTS["default"])
    stats.enable_stats(**HISTS["default"])
    ra, rc = _enable(both, steps, 600, par, arr, soc0), _enable(alone, steps, 600, par, arr, soc0)
    for s in (both, stats, alone):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) == _lib.OUT_SCHEDULE_SWEEP | _lib.OUT_FP64 and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and torch.equal(both.soc, alone.soc) and int(ra[0, :, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[0, :, 2].sum()) == int(ra[K - 1, :, 2].sum())


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "schedule sweep" before anything is launched: the
    chains' state and the batteries' stay as they were and the tables all zeros; what was enabled before still works."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.params import site_grid
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, arr, soc0 = PARAMS[:, :, :n], ARRAYS[:, :9], SOC0[:, :n]
    BAT = dict(capacity_wh=0.5, charge_w=1000.0, discharge_w=3000.0, charge_eff=0.95, discharge_eff=0.9, standby_w=1.0,
               soc0_wh=0.25)
    DSP = dict(BAT, charge_above_w=250.0, discharge_above_w=2000.0, feed_in_limit_w=500.0)
    RULES = [dict(charge_above_w=[0.0, 250.0, 500.0], feed_in_limit_w=[None, 500.0, 250.0]), dict(grid_charge_w=100.0)]
    SCH = dict(BAT, rules=[dict(charge_above_w=250.0), dict(grid_charge_w=100.0)], rule_of_interval=[0, 1] * 4 + [0])
    SW = dict(BAT, capacity_wh=[0.5, 0.25, 0.75], rules=RULES, rule_of_interval=[0, 1] * 4 + [0])

    def refused(sim, match, step0=0, k=100, trace=None, raw=None):
        before, soc = sim.state.clone(), sim.soc.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, None, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg and "schedule sweep" in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, None, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and torch.equal(soc, sim.soc)
        assert not bool((sim.schedule_sweep_raw if raw is None else raw).any())

    def desc(sim, **kw):
        """The sim's tmh_schedule_sweep with fields replaced."""
        d = sim._ssweep_desc
        f = dict(table=d.table, soc=d.soc, work=d.work, work_bytes=d.work_bytes, params=d.params,
                 rule_of_interval=d.rule_of_interval, n_rules=d.n_rules, n_variants=d.n_variants)
        return _lib.ScheduleSweep(**{**f, **kw})

    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, arr, soc0)
    out = torch.zeros(100, n, dtype=torch.float64, device="cuda:0")
    refused(sim, "schedule sweep tables are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # the sweep, then a fleet series
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    sim.enable_schedule_sweep(None)
    sim.enable_series(500)                                                 # a fleet series, then the sweep
    with pytest.raises(ValueError, match="fleet series"):
        _enable(sim, 500, 60, par, arr, soc0)
    sim.run(10, trace=())                                                  # the series still works
    torch.cuda.synchronize()
    assert int(sim.series_raw[0, :10, 2].sum()) > 0
    sim.enable_series(None)
    sim = _sim(n, start, prec=PREC, horizon=1000)
    buf = _enable(sim, 500, 60, par, arr, soc0)
    refused(sim, "outside the schedule sweep", step0=0, k=501)             # past the end
    _lib.check(L.tmh_set_schedule_sweep(sim._eng, C.byref(desc(sim, work_bytes=L.tmh_battery_sweep_work_bytes(n, 100, K) - 8))))
    refused(sim, "work buffer too small")                                  # enough for four variants of the window, not five
    p = buf.data_ptr()
    for kw, word in ((dict(table=_lib.Intervals(p + 4, 0, 500, 60, n)), b"8-byte aligned"),
                     (dict(table=_lib.Intervals(None, 0, 500, 60, n)), b"buffer"),
                     (dict(table=_lib.Intervals(p, 0, 500, 0, n)), b"interval_s"),
                     (dict(table=_lib.Intervals(p, 0, 500, 1 << 23, n)), b"2^23"),
                     (dict(n_variants=0), b"n_variants"), (dict(n_variants=17), b"n_variants"),
                     (dict(n_rules=0), b"n_rules"), (dict(n_rules=9), b"n_rules"),
                     (dict(soc=None), b"soc"), (dict(soc=sim.soc.data_ptr() + 4), b"soc"),
                     (dict(work=None), b"work"), (dict(work=p + 4), b"work"), (dict(work_bytes=K * 24 - 8), b"too small"),
                     (dict(params=None), b"params"), (dict(params=sim.schedule_sweep_params.data_ptr() + 4), b"params"),
                     (dict(rule_of_interval=None), b"rule_of_interval")):
        assert L.tmh_set_schedule_sweep(sim._eng, C.byref(desc(sim, **kw))) == -1 and word in L.tmh_last_error()
        assert b"schedule sweep" in L.tmh_last_error()                     # the setter refuses a bad struct
    # the sweep with another table kind on one engine -- the schedule and the other sweeps included -- in either order
    _enable(sim, 500, 60, par, arr, soc0)
    for kind, cols, word in (("intervals", 4, "the schedule sweep and interval metering"),
                             ("registers", 6, "the schedule sweep and the import / export registers"),
                             ("demand", 8, "the schedule sweep and the demand registers"),
                             ("storage", 9, "the schedule sweep and battery storage"),
                             ("battery", 10, "the schedule sweep and the battery kind"),
                             ("battery_sweep", 10, "the schedule sweep and the battery sweep"),
                             ("dispatch", 13, "the schedule sweep and battery dispatch"),
                             ("dispatch_sweep", 13, "the schedule sweep and the dispatch sweep"),
                             ("schedule", 13, "the schedule sweep and the schedule")):
        other = torch.zeros(9, cols, n, dtype=torch.int64, device="cuda:0")
        tbl = _lib.Intervals(other.data_ptr(), 0, 500, 60, n)
        d = sim._ssweep_desc
        arg = (_lib.Storage(tbl, d.soc, d.work, d.work_bytes, 100, 5, 5) if kind == "storage"
               else _lib.Battery(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "battery"
               else _lib.BatterySweep(tbl, d.soc, d.work, d.work_bytes, d.params, 1) if kind == "battery_sweep"
               else _lib.Dispatch(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "dispatch"
               else _lib.DispatchSweep(tbl, d.soc, d.work, d.work_bytes, d.params, 1) if kind == "dispatch_sweep"
               else _lib.Schedule(tbl, d.soc, d.work, d.work_bytes, d.params, d.rule_of_interval, d.n_rules) if kind == "schedule"
               else tbl)
        setter = getattr(L, "tmh_set_" + kind)
        _lib.check(setter(sim._eng, C.byref(arg)))
        refused(sim, word)
        _lib.check(L.tmh_set_schedule_sweep(sim._eng, None))
        _lib.check(L.tmh_set_schedule_sweep(sim._eng, C.byref(sim._ssweep_desc)))   # (now the sweep after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
        extra = (A_BATTERY if kind == "storage" else BAT if kind in ("battery", "battery_sweep") else SCH if kind == "schedule"
                 else DSP if kind in ("dispatch", "dispatch_sweep") else {})
        with pytest.raises(ValueError, match="the schedule sweep"):
            getattr(sim, "enable_" + kind)(500, 60, **extra)
        o = _sim(64, start, prec=PREC, horizon=1000)
        oraw = getattr(o, "enable_" + kind)(500, 60, **extra)
        with pytest.raises(ValueError, match="one table output per sim"):
            o.enable_schedule_sweep(500, 60, **SW)
        o.run(60, trace=())                                                # the table enabled before still works
        torch.cuda.synchronize()
        first = oraw[0, 0, 2] if kind.endswith("_sweep") else oraw[0, 2]
        assert int(first.sum()) > 0 and o.schedule_sweep_raw is None
    # the battery fleet series and the dispatch fleet series: other kinds' outputs, in either order
    for name, cols in (("battery_fleet", 8), ("dispatch_fleet", 9)):
        fl = torch.zeros(1, 500, cols, dtype=torch.int64, device="cuda:0")
        setter = getattr(L, "tmh_set_" + name)
        _lib.check(setter(sim._eng, C.byref(_lib.Series(fl.data_ptr(), 0, 500, 0, 1, 0))))
        refused(sim, name.replace("_", " ") + " series")
        _lib.check(L.tmh_set_schedule_sweep(sim._eng, None))
        _lib.check(L.tmh_set_schedule_sweep(sim._eng, C.byref(sim._ssweep_desc)))
        refused(sim, name.replace("_", " ") + " series")
        assert not bool(fl.any())
        _lib.check(setter(sim._eng, None))
    o = _sim(64, start, prec=PREC, horizon=1000)
    o.enable_schedule(500, 60, **SCH)
    o.enable_dispatch_fleet(500)
    with pytest.raises(ValueError, match="one table output per sim|dispatch fleet series"):
        o.enable_schedule_sweep(500, 60, **SW)
    o.run(60, trace=())
    torch.cuda.synchronize()
    assert int(o.dispatch_fleet_raw[0, :60, 2].sum()) > 0 and int(o.schedule_raw[0, 2].sum()) > 0
    # per-chain sites
    ss = _sim(64, start, prec=PREC, horizon=1000, sites=site_grid(8, 8))
    with pytest.raises(ValueError, match="per-chain sites"):
        ss.enable_schedule_sweep(500, 60, **SW)
    sraw = torch.zeros(K, 9, 13, 64, dtype=torch.int64, device="cuda:0")
    ssoc, spar, sarr = _dev(SOC0[:, :64]), _dev(PARAMS[:, :, :64]), _dev(arr)
    swork = torch.empty(L.tmh_battery_sweep_work_bytes(64, 500, K), dtype=torch.uint8, device="cuda:0")
    sdesc = _lib.ScheduleSweep(_lib.Intervals(sraw.data_ptr(), 0, 500, 60, 64), ssoc.data_ptr(), swork.data_ptr(), swork.numel(),
                               spar.data_ptr(), sarr.data_ptr(), R, K)
    _lib.check(L.tmh_set_schedule_sweep(ss._eng, C.byref(sdesc)))
    ss.soc = ssoc
    refused(ss, "per-chain sites", raw=sraw)
    _lib.check(L.tmh_set_schedule_sweep(ss._eng, None))
    # fp32 engines: refused at the setter and at enable_schedule_sweep
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    with pytest.raises(ValueError, match="fp64"):
        f32.enable_schedule_sweep(500, 60, **SW)
    assert L.tmh_set_schedule_sweep(f32._eng, C.byref(sim._ssweep_desc)) == -1
    assert b"fp64" in L.tmh_last_error() and b"schedule sweep" in L.tmh_last_error()
    # the Python layer refuses values outside their ranges, arrays of the wrong shape and entries at or above R
    for bad in (dict(capacity_wh=1e9), dict(charge_eff=0.4), dict(soc0_wh=0.6), dict(charge_w=[1.0, 2.0]), dict(n_variants=4),
                dict(n_rules=3), dict(rule_of_interval=None), dict(rule_of_interval=[0, 1] * 4), dict(rule_of_interval=[0, 2] * 4 + [0]),
                dict(rule_of_interval=np.zeros((2, 9), np.uint8)), dict(rules=[dict(grid_charge_w=-1.0)]), dict(rules=None)):
        with pytest.raises(ValueError):
            sim.enable_schedule_sweep(500, 60, **{**SW, **bad})
    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_schedule_sweep(500, 60, **SW)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the schedule sweep"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.schedule_sweep_raw.any())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw, hostpar = _np(sim.schedule_sweep_raw), _np(sim.schedule_sweep_params)
    assert raw.shape == (3, 9, 13, n) and hostpar.shape == (3, 14, n) and (hostpar[2, 8] == 250 << 12).all()
    for v in range(3):
        assert int(raw[v, :2, 2].sum()) > 0 and not raw[v, 2:].any()
        identities(raw[v], limit_params(hostpar[v], [0, 1] * 4 + [0]))
    assert L.tmh_set_schedule_sweep(sim._eng, None) == 0                   # NULL: off
