"""Scheduled dispatch on the GPU (tmh_set_schedule, BatchedSim.enable_schedule; fp64 throughout): integers, so
every comparison with the traces' table (schedule.from_traces, a plain loop over the seconds) is bit for bit.
The expected table and state of charge always come from traces of separate sims of the same chains
(test_gpu_storage.a60_gpu / c60_traces: computed once, shared with the storage, battery and dispatch tests) or
from the dispatch kind's own kernels, never from the kernels under test.  The households and the tariff are
schedule_util.recipe's: battery_util's per-chain batteries, four rule sets per chain (one of them charging from
the grid, one holding) and a rule per metering interval."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from battery_util import QUARTER_WH
from dispatch_util import identities, soc_changes
from schedule_util import A_FLOORS, A_RULES, NO_LIMIT, R, c_rules, limits, recipe, run, tiled
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


def _enable(sim, n_steps, interval_s, params=PARAMS, rules=A_RULES, soc0=SOC0, **kw):
    """enable_schedule with ready parameters, the rule array and a caller-owned soc (the recipe's by default)."""
    return sim.enable_schedule(n_steps, interval_s, params=_dev(params), rule_of_interval=rules, soc=_dev(soc0), **kw)


def _limit_params(params, rules):
    """dispatch_util.identities' argument with the limit in force per interval in row 8."""
    lim = limits(params, rules)
    fake = np.zeros((9,) + lim.shape, dtype=np.int64)
    fake[8] = lim
    return fake


@functools.lru_cache(maxsize=None)
def a_want():
    """The expected table and end state of input A with the recipe's households, from the storage tests' traces."""
    from tmhpvsim_amd import schedule
    t = a60_gpu()
    return schedule.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS, rule_of_interval=A_RULES, soc0=SOC0)


@functools.lru_cache(maxsize=None)
def a_sc():
    """The schedule sim of input A, one tmh_run per window of A_WINDOWS."""
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, A_STEPS, IV)
    assert tuple(raw.shape) == (13, 13, A_N) and tuple(sim.soc.shape) == (A_N,) and sim.soc.dtype == torch.int64
    assert tuple(sim.schedule_params.shape) == (6 + 4 * R, A_N) and sim.schedule_raw is raw
    assert sim.schedule_rules.dtype == torch.uint8 and _np(sim.schedule_rules).tolist() == A_RULES.tolist()
    variants, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), soc=_np(sim.soc), variants=variants, guards=guards, status=sim.status())


def test_schedule_equals_the_traces_table():
    """The main test: all thirteen columns and the state of charge bit for bit, over two windows (the second off
    the four-step grid), twelve interval boundaries of which eleven change the rule, chains faulted at
    construction and inside the window, grid charging into empty and full batteries, hold intervals."""
    from tmhpvsim_amd import _lib
    g, t = a_sc(), a60_gpu()
    want, end = a_want()
    a_has_teeth(t["pv"], t["cov"], g["status"])
    _, _, ev = run(t["pv"], t["meter"], t["cov"], IV, PARAMS, A_RULES, SOC0)
    dead = g["status"] == 1
    print(ev, "dead at construction", int(dead.sum()), "in-window faults", int(((t["cov"][-1] == 255) & ~dead).sum()))
    for name, floor in A_FLOORS.items():
        assert ev[name] >= floor, (name, ev[name], floor)
    assert g["variants"] == [_lib.OUT_SCHEDULE | _lib.OUT_FP64] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    for col in range(13):
        np.testing.assert_array_equal(g["raw"][:, col], want[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(g["soc"], end)
    assert dead.any() and not g["raw"][:, :, dead].any() and (g["soc"][dead] == SOC0[dead]).all()
    identities(g["raw"], _limit_params(PARAMS, A_RULES))
    soc_changes(g["raw"], SOC0, g["soc"])
    assert g["raw"][12, 2].max() == 3 and g["raw"][:12, 2].max() == IV          # the last partial interval


def test_windows_pipelining_and_compaction_same_bits():
    """One tmh_run per window (a_sc), one pipelined run over windows of 4,000 steps, and compacted windows of
    3,601 steps (from the second window on only the live chains run, in dense slots: a slot's work column is the
    slot's; its soc, its table column and its rules' parameters are the chain's, ids[slot]): the same bits."""
    g = a_sc()
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
    for row in [r for r in range(6 + 4 * R) if len(set(PARAMS[r].tolist())) > 1]:   # indexed by slot: other chains'
        assert (PARAMS[row, ids] != PARAMS[row, :len(ids)]).any(), row
    np.testing.assert_array_equal(_np(raw), g["raw"])
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    np.testing.assert_array_equal(sim.status(), g["status"])


@pytest.mark.parametrize("interval_s", [7, 128])
@pytest.mark.parametrize("n", [1300, 64])
def test_schedule_boundaries(n, interval_s):
    """Rule changes inside four-second groups (7: eighteen per 128-s block) and one per block, off the block grid by
    three (128); the origin three steps before the run, so no interval edge coincides with a window edge; a partial
    wavefront and construction faults; the C recipe (thresholds, limits and grid powers that bind just after
    sunrise) tiled past A_N.  The map pass must take each second's rule from the second's own interval."""
    from tmhpvsim_amd import _lib, demand, schedule
    pv, meter, cov = c60_traces(n)
    par, soc0 = tiled(n, "C")
    rules = c_rules(-(-(C_STEPS + C_LEAD) // interval_s))
    want, end, ev = run(pv, meter, cov, interval_s, par, rules, soc0, origin=C_LEAD)
    print(f"n {n}: {ev}, construction faults {int((cov[0] == 255).sum())}")
    for name, count in ev.items():
        assert count > 0 or (name == "grid_partial_fill" and n == 64), name
    if n > 1000:
        assert (cov[0] == 255).any()                                                       # construction faults
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, C_STEPS + C_LEAD, interval_s, par, rules, soc0, step0=-C_LEAD)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_SCHEDULE | _lib.OUT_FP64
    torch.cuda.synchronize()
    ref, rend = schedule.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, params=par, rule_of_interval=rules, soc0=soc0)
    np.testing.assert_array_equal(ref, want)                      # (the two derivations agree on this input too)
    assert tuple(raw.shape) == want.shape == (-(-(C_STEPS + C_LEAD) // interval_s), 13, n)
    for w0 in np.cumsum((0,) + C_WINDOWS)[:-1]:                   # where a window begins (and the one before it ends)
        assert (int(w0) + C_LEAD) % interval_s != 0
    got = _np(raw)
    np.testing.assert_array_equal(_np(sim.soc), end, err_msg="soc")
    for col in range(13):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(rend, end)
    identities(got, _limit_params(par, rules))
    soc_changes(got, soc0, _np(sim.soc))
    live0 = want[0, 2] == interval_s - C_LEAD                     # the first cell begins at offset C_LEAD
    assert live0.any()
    for col in (11, 12):
        assert (demand.unpack(got[0, col, live0])[1] >= C_LEAD).all()


@functools.lru_cache(maxsize=None)
def a_dispatch_rule0():
    """Input A under rule 0 throughout by the dispatch kind's own kernels: its table and end state."""
    from tmhpvsim_amd import _lib, schedule
    dp = _sim(A_N, A_START, **_kw60())
    rd = dp.enable_dispatch(A_STEPS, IV, params=_dev(schedule.to_dispatch_params(PARAMS, 0)), soc=_dev(SOC0))
    _run_windows(dp, A_WINDOWS)
    assert _last(dp) == _lib.OUT_DISPATCH | _lib.OUT_FP64
    return _np(rd), _np(dp.soc)


@pytest.mark.parametrize("case", ["one_rule", "equal_rules", "one_rule_throughout"])
def test_reduces_to_the_dispatch_kind(case):
    """R = 1; R = 4 with all of a chain's rules equal; and an array that names rule 0 throughout: thirteen columns
    and soc of an enable_dispatch sim of the same households, the parent's kernels as the reference."""
    from tmhpvsim_amd import _lib
    want, end = a_dispatch_rule0()
    par, rules = {"one_rule": (PARAMS[:10], np.zeros(13, np.uint8)),
                  "equal_rules": (np.vstack([PARAMS[:6]] + [PARAMS[6:10]] * R), A_RULES),
                  "one_rule_throughout": (PARAMS, np.zeros(13, np.uint8))}[case]
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV, par, rules)
    _run_windows(sim, A_WINDOWS)
    assert _last(sim) == _lib.OUT_SCHEDULE | _lib.OUT_FP64
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    assert int(want[:, 6].sum()) > 0 and int(want[:, 7].sum()) > 0 and int(want[:, 10].sum()) > 0


def test_dispatch_kind_as_reference_across_a_rule_change():
    """A rule change at a window edge, without grid charging: windows of 4,500 and 6,303 steps, rule 0 in the first
    five intervals and the recipe's rule 3 after -- against one enable_dispatch sim run over the same two windows
    with its params rows 6-8 overwritten in place between them."""
    from tmhpvsim_amd import schedule
    wins = (4500, A_STEPS - 4500)
    assert wins[0] % IV == 0 and wins[1] == 6303
    par = np.vstack([PARAMS[:10], PARAMS[18:22]])
    assert not par[9].any() and not par[13].any() and (par[6:9] != par[10:13]).any()
    rules = np.array([0] * 5 + [1] * 8, dtype=np.uint8)
    dp = _sim(A_N, A_START, **_kw60())
    dpar = _dev(schedule.to_dispatch_params(par, 0))
    rd = dp.enable_dispatch(A_STEPS, IV, params=dpar, soc=_dev(SOC0))
    dp.run(wins[0], trace=(), window=wins[0])
    torch.cuda.synchronize()
    dpar[6:9] = _dev(par[10:13])                                  # rule 1 from here on
    dp.run(wins[1], trace=(), window=wins[1])
    torch.cuda.synchronize()
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV, par, rules)
    _run_windows(sim, wins)
    np.testing.assert_array_equal(_np(raw), _np(rd))
    np.testing.assert_array_equal(_np(sim.soc), _np(dp.soc))
    t = a60_gpu()
    want, end = schedule.from_traces(t["pv"], t["meter"], t["cov"], IV, params=par, rule_of_interval=rules, soc0=SOC0)
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    assert (want != a_dispatch_rule0()[0]).any()                  # the second rule changed something


def test_two_batches_fill_one_table():
    """Chains [5000, 5500) and [5500, 6000) as two sims writing column slices of one table, reading slices of
    one [6 + 4 R, 1000] params tensor and the one rule array, and carrying slices of one soc."""
    want, end = a_want()
    big = torch.zeros(13, 13, A_N, dtype=torch.int64, device="cuda:0")
    params, soc, rules = _dev(PARAMS), _dev(SOC0), _dev(A_RULES)
    for a, b in ((0, 500), (500, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        view = big[:, :, a:b]
        got = s.enable_schedule(A_STEPS, IV, buffer=view, soc=soc[a:b], params=params[:, a:b], rule_of_interval=rules, n_rules=R)
        assert got is view and s._schedule.ld == A_N and s.soc.data_ptr() == soc[a:b].data_ptr()
        assert s.schedule_params.data_ptr() == params[:, a:b].data_ptr() and s.schedule_rules.data_ptr() == rules.data_ptr()
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), want)
    np.testing.assert_array_equal(_np(soc), end)
    np.testing.assert_array_equal(_np(params), PARAMS)                                     # read only
    np.testing.assert_array_equal(_np(rules), A_RULES)
    kw = dict(rule_of_interval=rules)
    with pytest.raises(ValueError, match="strides"):
        s.enable_schedule(A_STEPS, IV, buffer=big[:, :, :2 * s.n:2], params=params[:, 500:], **kw)   # chains not contiguous
    with pytest.raises(ValueError, match="schedule buffer"):
        s.enable_schedule(A_STEPS, IV, buffer=torch.zeros(13, 10, s.n, dtype=torch.int64, device="cuda:0"),
                          params=params[:, 500:], **kw)
    with pytest.raises(ValueError, match="row stride"):                                    # params of another width than the table
        s.enable_schedule(A_STEPS, IV, params=params[:, 500:], **kw)
    with pytest.raises(ValueError, match="params"):
        s.enable_schedule(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:, :2 * s.n:2], **kw)
    with pytest.raises(ValueError, match="params"):                                        # battery dispatch's nine rows
        s.enable_schedule(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:9, 500:], **kw)
    with pytest.raises(ValueError, match="n_rules"):
        s.enable_schedule(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:, 500:], n_rules=3, **kw)
    with pytest.raises(ValueError, match="soc"):
        s.enable_schedule(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:, 500:], soc=soc[:2 * s.n:2], **kw)
    assert s.schedule_raw is view and s.schedule_params.data_ptr() == params[:, 500:].data_ptr()   # as it was
    s.enable_schedule(None)
    assert s.soc is None and s.schedule_raw is None and s.schedule_params is None and s.schedule_rules is None


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_statistics_unperturbed_by_the_schedule(spec):
    """Statistics beside the schedule table are the statistics-only run's, bit for bit (the map pass adds nothing
    to them), and the table is the schedule-only one."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw60(steps)
    par, soc0, rules = PARAMS[:, :n], SOC0[:n], np.array([1, 3, 2], dtype=np.uint8)
    both, stats, alone = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats(**HISTS[spec])
    stats.enable_stats(**HISTS[spec])
    ra, rc = _enable(both, steps, 600, par, rules, soc0), _enable(alone, steps, 600, par, rules, soc0)
    for s in (both, stats, alone):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) == _lib.OUT_SCHEDULE | _lib.OUT_FP64 and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and torch.equal(both.soc, alone.soc) and int(ra[:, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[:, 2].sum())
    assert int(ra[:, 6].sum()) > 0 and int(ra[:, 9].sum()) > 0
    identities(_np(ra), _limit_params(par, rules))


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "schedule" before anything is launched: the
    chains' state and the batteries' stay as they were and the table all zeros; after all of them the sim runs."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams, site_grid
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    rules = np.array([1, 0, 2, 3, 0, 1, 1, 3, 2], dtype=np.uint8)               # 500 steps of 60 s: nine intervals
    BAT = dict(capacity_wh=0.5, charge_w=1000.0, discharge_w=3000.0, charge_eff=0.95, discharge_eff=0.9, standby_w=1.0,
               soc0_wh=0.25)
    DSP = dict(BAT, charge_above_w=250.0, discharge_above_w=2000.0, feed_in_limit_w=500.0)
    SCH = dict(BAT, rules=[dict(charge_above_w=250.0, discharge_above_w=2000.0, feed_in_limit_w=500.0),
                           dict(grid_charge_w=100.0)], rule_of_interval=[0, 1, 0, 1, 1, 0, 0, 1, 0])

    def refused(sim, match, step0=0, k=100, trace=None, inj=None):
        before, soc = sim.state.clone(), sim.soc.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        ij = C.byref(inj) if inj is not None else None
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg and "schedule" in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if sim.path == "time_parallel" and trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and torch.equal(soc, sim.soc)
        assert not bool(sim.schedule_raw.any())

    def desc(sim, **kw):
        """The sim's tmh_schedule with fields replaced."""
        d = sim._schedule_desc
        f = dict(table=d.table, soc=d.soc, work=d.work, work_bytes=d.work_bytes, params=d.params,
                 rule_of_interval=d.rule_of_interval, n_rules=d.n_rules)
        return _lib.Schedule(**{**f, **kw})

    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, rules, soc0)
    out = torch.zeros(100, n, dtype=torch.float64, device="cuda:0")
    refused(sim, "schedule tables are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # the schedule, then a fleet series
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    sim.enable_schedule(None)
    sim.enable_series(500)                                                 # a fleet series, then the schedule
    with pytest.raises(ValueError, match="fleet series"):
        _enable(sim, 500, 60, par, rules, soc0)
    sim.enable_series(None)
    _enable(sim, 500, 60, par, rules, soc0)
    fl = torch.zeros(1, 500, 8, dtype=torch.int64, device="cuda:0")        # the battery fleet series beside the schedule
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(_lib.Series(fl.data_ptr(), 0, 500, 0, 1, 0))))
    refused(sim, "battery fleet series")
    assert not bool(fl.any())
    _lib.check(L.tmh_set_battery_fleet(sim._eng, None))
    with pytest.raises(ValueError, match="enable_battery first"):
        sim.enable_battery_fleet(500)
    refused(sim, "outside the schedule tables", step0=0, k=501)            # past the end
    refused(sim, "outside the schedule tables", step0=450, k=100)
    _enable(sim, 500, 60, par, rules, soc0, step0=10)
    refused(sim, "outside the schedule tables", step0=0, k=100)            # before the origin
    buf = _enable(sim, 500, 60, par, rules, soc0)
    _lib.check(L.tmh_set_schedule(sim._eng, C.byref(desc(sim, table=_lib.Intervals(buf.data_ptr(), 0, 500, 60, n - 1)))))
    refused(sim, "schedule tables ld")                                     # ld too small
    _lib.check(L.tmh_set_schedule(sim._eng, C.byref(desc(sim, work_bytes=L.tmh_storage_work_bytes(n, 100) - 8))))
    refused(sim, "work buffer too small")
    p = buf.data_ptr()
    for kw, word in ((dict(table=_lib.Intervals(p + 4, 0, 500, 60, n)), b"8-byte aligned"),
                     (dict(table=_lib.Intervals(None, 0, 500, 60, n)), b"buffer"),
                     (dict(table=_lib.Intervals(p, 0, 500, 0, n)), b"interval_s"),
                     (dict(table=_lib.Intervals(p, 0, 0, 60, n)), b"n_steps"),
                     (dict(table=_lib.Intervals(p, 0, 500, 60, 0)), b"ld"),
                     (dict(table=_lib.Intervals(p, 0, 500, 1 << 23, n)), b"2^23"),
                     (dict(soc=None), b"soc"), (dict(soc=sim.soc.data_ptr() + 4), b"soc"),
                     (dict(work=None), b"work"), (dict(work=p + 4), b"work"), (dict(work_bytes=16), b"work buffer too small"),
                     (dict(params=None), b"params"), (dict(params=sim.schedule_params.data_ptr() + 4), b"params"),
                     (dict(n_rules=0), b"n_rules"), (dict(n_rules=9), b"n_rules"),
                     (dict(rule_of_interval=None), b"rule_of_interval")):
        assert L.tmh_set_schedule(sim._eng, C.byref(desc(sim, **kw))) == -1 and word in L.tmh_last_error(), kw
        assert b"schedule" in L.tmh_last_error()                           # the setter refuses a bad struct
    # the schedule with another table kind on one engine, in either order: every kind, both sweeps included
    _enable(sim, 500, 60, par, rules, soc0)
    for kind, cols, word in (("intervals", 4, "the schedule and interval metering"),
                             ("registers", 6, "the schedule and the import / export registers"),
                             ("demand", 8, "the schedule and the demand registers"),
                             ("storage", 9, "the schedule and battery storage"),
                             ("battery", 10, "the schedule and the battery kind"),
                             ("battery_sweep", 10, "the schedule and the battery sweep"),
                             ("dispatch", 13, "the schedule and battery dispatch"),
                             ("dispatch_sweep", 13, "the schedule and the dispatch sweep")):
        other = torch.zeros(9, cols, n, dtype=torch.int64, device="cuda:0")
        tbl = _lib.Intervals(other.data_ptr(), 0, 500, 60, n)
        d = sim._schedule_desc
        arg = (_lib.Storage(tbl, d.soc, d.work, d.work_bytes, 100, 5, 5) if kind == "storage"
               else _lib.Battery(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "battery"
               else _lib.Dispatch(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "dispatch"
               else _lib.BatterySweep(tbl, d.soc, d.work, d.work_bytes, d.params, 1) if kind == "battery_sweep"
               else _lib.DispatchSweep(tbl, d.soc, d.work, d.work_bytes, d.params, 1) if kind == "dispatch_sweep" else tbl)
        setter = getattr(L, "tmh_set_" + kind)
        _lib.check(setter(sim._eng, C.byref(arg)))
        refused(sim, word)
        _lib.check(L.tmh_set_schedule(sim._eng, None))
        _lib.check(L.tmh_set_schedule(sim._eng, C.byref(sim._schedule_desc)))   # (now the schedule after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
        kw = (A_BATTERY if kind == "storage" else BAT if kind in ("battery", "battery_sweep")
              else DSP if kind in ("dispatch", "dispatch_sweep") else {})
        with pytest.raises(ValueError, match="the schedule"):
            getattr(sim, "enable_" + kind)(500, 60, **kw)
        o = _sim(64, start, prec=PREC, horizon=1000)
        getattr(o, "enable_" + kind)(500, 60, **kw)
        with pytest.raises(ValueError, match="one table output per sim"):
            o.enable_schedule(500, 60, **SCH)
        o.run(100, trace=())                                               # what was enabled before still runs
        torch.cuda.synchronize()
        assert int(getattr(o, kind + "_raw").abs().sum()) > 0 and o.schedule_raw is None
    seq = _sim(64, start, prec=PREC, horizon=1000, kernel_path="sequential")   # the sequential path
    seq.enable_schedule(500, 60, **SCH)
    refused(seq, "schedule tables need the time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), precision=PREC, device="cuda:0",
                      injected=inj, horizon=1000)
    isim.enable_schedule(500, 60, **SCH)
    refused(isim, "time-parallel", inj=isim._us)
    mp = ModelParams()
    mp.inverter = dict(mp.inverter, Paco=float(L.tmh_series_max_w()))      # Paco >= TMH_SERIES_MAX_W
    big = _sim(64, start, prec=PREC, mp=mp, horizon=1000)
    big.enable_schedule(500, 60, **SCH)
    refused(big, "TMH_SERIES_MAX_W")
    # per-chain sites: refused at enable_schedule and, set behind its back, at the step
    sited = _sim(64, start, prec=PREC, horizon=1000, sites=site_grid(8, 8))
    with pytest.raises(ValueError, match="per-chain sites"):
        sited.enable_schedule(500, 60, **SCH)
    s64 = _sim(64, start, prec=PREC, horizon=1000)
    s64.enable_schedule(500, 60, **SCH)
    si = torch.from_numpy(np.ascontiguousarray(_np(sited.sites[0]))).to("cuda:0")
    _lib.check(L.tmh_set_sites(s64._eng, C.c_void_p(si.data_ptr()), None, 64))
    refused(s64, "per-chain sites")
    _lib.check(L.tmh_set_sites(s64._eng, None, None, 0))
    # fp32 engines: refused at the setter and at enable_schedule
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    with pytest.raises(ValueError, match="fp64"):
        f32.enable_schedule(500, 60, **SCH)
    assert L.tmh_set_schedule(f32._eng, C.byref(sim._schedule_desc)) == -1
    assert b"fp64" in L.tmh_last_error() and b"schedule" in L.tmh_last_error()
    # the Python layer refuses values outside their ranges before upload, a soc0 outside [0, C], and a bad rule array
    kept = sim.schedule_raw
    for bad in (dict(capacity_wh=1e9), dict(charge_w=-1.0), dict(charge_eff=0.4), dict(soc0_wh=0.6), dict(soc0_wh=-0.1),
                dict(capacity_wh=[0.5] * 7)):                              # (the battery's rows: battery.quantize_params' words)
        with pytest.raises(ValueError):
            sim.enable_schedule(500, 60, **{**SCH, **bad})
    for bad in (dict(rules=[dict(grid_charge_w=-1.0)]), dict(rules=[dict(charge_above_w=40000.0)]),
                dict(rules=[dict(feed_in_limit_w=float("nan"))]), dict(rules=[]), dict(rules=[dict()] * 9),
                dict(rule_of_interval=[0, 1, 0, 1, 1, 0, 0, 1]), dict(rule_of_interval=[0, 1, 0, 1, 1, 0, 0, 1, 2]),
                dict(rule_of_interval=None), dict(rule_of_interval=[0.5] * 9), dict(n_rules=3)):
        with pytest.raises(ValueError, match="schedule"):
            sim.enable_schedule(500, 60, **{**SCH, **bad})
    worse = par.copy()
    worse[9, 5] = (1 << 27) + 1
    with pytest.raises(ValueError, match="grid_charge"):
        sim.enable_schedule(500, 60, params=_dev(worse), rule_of_interval=rules)
    with pytest.raises(ValueError, match="required"):
        sim.enable_schedule(500, 60, rule_of_interval=rules)
    assert sim.schedule_raw is kept and kept is not None                   # the schedule enabled before is still there

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_schedule(500, 60, **SCH)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the schedule"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.schedule_raw.any())
    assert bool((sim.soc == QUARTER_WH).all())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw = _np(sim.schedule_raw)
    assert int(raw[0, 2].min()) >= 0 and int(raw[:2, 2].sum()) > 0
    assert not raw[2:].any()
    identities(raw, _limit_params(_np(sim.schedule_params), _np(sim.schedule_rules)))
    soc_changes(raw, np.full(n, QUARTER_WH), _np(sim.soc))
    assert L.tmh_set_schedule(sim._eng, None) == 0                         # NULL: off


def test_schedule_cli(tmp_path):
    from click.testing import CliRunner
    from tmhpvsim_amd import schedule
    from tmhpvsim_amd.cli import TABLE_CSV, main
    f, z = tmp_path / "sc.csv", tmp_path / "sc.npz"
    r = CliRunner().invoke(main, ["schedule", str(f), "--batch", "64", "--seconds", "1900", "--interval", "600",
                                  "--no-realtime", "--capacity-wh", "0.5,0,0.25", "--charge-w", "1000", "--discharge-w",
                                  "3000,1500", "--charge-eff", "0.95", "--discharge-eff", "0.9,1.0", "--standby-w", "2",
                                  "--soc0-wh", "0.25,0,0.25", "--period", "00:00,20,100,10,0", "--period",
                                  "12:10,0,0,none,50", "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["time"] + [name for name, _ in TABLE_CSV["dispatch"]] + ["rule"] and len(rows) == 1 + 4
    saved = np.load(z)
    raw = saved["raw"]
    assert raw.shape == (4, 13, 64) and int(saved["interval_s"]) == 600 and saved["rule"].tolist() == [0, 1, 1, 1]
    assert [row[-1] for row in rows[1:]] == ["0", "1", "1", "1"]
    assert [row[0] for row in rows[1:]] == ["2019-09-06 12:00:00", "2019-09-06 12:10:00", "2019-09-06 12:20:00",
                                            "2019-09-06 12:30:00"]
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0] + raw[:, 6] - raw[:, 7] + raw[:, 10])
    lim = np.array([10 << 12] + [NO_LIMIT] * 3, dtype=np.int64)[:, None]
    assert ((raw[:, 12] >> 32) <= lim).all() and int(raw[0, 10].sum()) > 0 and not raw[1:, 10].any()
    assert not raw[1:, 7].any() and raw[3, 2].max() == 100                 # the grid rule never discharges; a partial interval
    has = np.arange(64) % 3 != 1                                           # chains with a battery
    assert int(raw[1:, 6][:, has].sum()) > 0 and not raw[1:, 6][:, ~has].any()
    want = schedule.to_watts(raw[:, :, :1], 600, n_steps=1900)             # column 0: chain 0
    for k, row in enumerate(rows[1:]):
        assert [float(x) for x in row[1:-1]] == [float(want[key][k, 0]) for _, key in TABLE_CSV["schedule"]]
    full = schedule.to_watts(raw, 600, n_steps=1900)
    for key in full:
        np.testing.assert_array_equal(saved[key], full[key], err_msg=key)
