"""The dispatch fleet series on the GPU (tmh_set_dispatch_fleet, BatchedSim.enable_dispatch_fleet; fp64 throughout)
behind battery dispatch and behind the schedule: integers, so every comparison with the traces' rows
(dispatch.fleet_from_traces, schedule.fleet_from_traces: plain loops over the seconds) is bit for bit.  The expected
rows always come from traces of separate sims of the same chains (test_gpu_storage.a60_gpu / c60_traces: computed
once, shared with the storage, battery, dispatch and schedule tests) or from existing kernels (the kinds' runs
without the series, the battery fleet series, the schedule against dispatch), never from the kernels under test.
The households are dispatch_util.recipe's and schedule_util.recipe's."""
import ctypes as C
import functools

import numpy as np
import pytest

import dispatch_util
import schedule_util
from range_util import corners
from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_WINDOWS, a_has_teeth
from storage_util import modules_params
from test_gpu_registers import C_START, C_STEPS, _run_windows
from test_gpu_series import _last, _np, _sim
from test_gpu_storage import IV, PREC, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

D_PARAMS, D_SOC0 = dispatch_util.recipe()
S_PARAMS, S_SOC0 = schedule_util.recipe()
A_RULES = schedule_util.A_RULES
GC = 512
KINDS = ["dispatch", "schedule"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _enable(sim, kind, n_steps, interval_s, params=None, soc0=None, rules=None, **kw):
    """enable_dispatch or enable_schedule with ready parameters (the kind's recipe by default) and a caller-owned soc."""
    if kind == "dispatch":
        return sim.enable_dispatch(n_steps, interval_s, params=_dev(D_PARAMS if params is None else params),
                                   soc=_dev(D_SOC0 if soc0 is None else soc0), **kw)
    return sim.enable_schedule(n_steps, interval_s, params=_dev(S_PARAMS if params is None else params),
                               rule_of_interval=A_RULES if rules is None else rules, soc=_dev(S_SOC0 if soc0 is None else soc0), **kw)


def _code(kind):
    from tmhpvsim_amd import _lib
    return (_lib.OUT_DISPATCH_FLEET if kind == "dispatch" else _lib.OUT_SCHEDULE_FLEET) | _lib.OUT_FP64


def _ref(kind, pv, meter, cov, interval_s=IV, params=None, soc0=None, rules=None, origin=0, gc=GC):
    from tmhpvsim_amd import dispatch, schedule
    if kind == "dispatch":
        return dispatch.fleet_from_traces(pv, meter, cov, params=D_PARAMS if params is None else params,
                                          soc0=D_SOC0 if soc0 is None else soc0, group_chains=gc)
    return schedule.fleet_from_traces(pv, meter, cov, interval_s, params=S_PARAMS if params is None else params,
                                      rule_of_interval=A_RULES if rules is None else rules, soc0=S_SOC0 if soc0 is None else soc0,
                                      origin=origin, group_chains=gc)


def _row_identities(raw, cap_sum=None):
    """Columns 4-8 >= 0, the discharging power [7] - sum of b >= 0 with sum of b from [4] - [5] - [8] == [1] - [0] + sum
    of b, the counts consistent, and [6] <= the sum of the capacities."""
    assert (raw[..., 4:] >= 0).all() and (raw[..., 2] >= raw[..., 3]).all() and (raw[..., 3] >= 0).all()
    sb = raw[..., 4] - raw[..., 5] - raw[..., 8] - (raw[..., 1] - raw[..., 0])
    assert (raw[..., 7] - sb >= 0).all()
    if cap_sum is not None:
        assert (raw[..., 6].T <= np.asarray(cap_sum)).all()


def _columns_equal(got, want):
    differ = [int((got[..., col] != want[..., col]).sum()) for col in range(9)]   # (group, second) rows per column
    print("rows that differ per column", differ, "of", got.shape[0] * got.shape[1])
    assert differ == [0] * 9


@functools.lru_cache(maxsize=None)
def a_want(kind):
    """The expected rows of input A in groups of 512 and the end state, from the storage tests' traces."""
    t = a60_gpu()
    want, end = _ref(kind, t["pv"], t["meter"], t["cov"])
    want.setflags(write=False)
    return want, end


@functools.lru_cache(maxsize=None)
def a_fl(kind):
    """The kind's sim of input A with the dispatch fleet series, one tmh_run per window of A_WINDOWS."""
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, kind, A_STEPS, IV)
    fl = sim.enable_dispatch_fleet(A_STEPS, group_chains=GC)
    assert fl is sim.dispatch_fleet_raw and tuple(fl.shape) == (2, A_STEPS, 9) and fl.dtype == torch.int64
    variants, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), fleet=_np(fl), soc=_np(sim.soc), variants=variants, guards=guards, status=sim.status())


def _a_table(kind):
    """The kind's table and end state of input A by its run without the series (the dispatch and the schedule tests')."""
    if kind == "dispatch":
        from test_gpu_dispatch import a_dp
        return a_dp()
    from test_gpu_schedule import a_sc
    return a_sc()


@pytest.mark.parametrize("kind", KINDS)
def test_fleet_equals_the_traces_rows(kind):
    """The main test: all nine columns of both groups (512 chains and a partial group of 488) bit for bit over two
    windows (the second off the four-step grid; under the schedule eleven rule changes, grid charging and hold
    intervals), the kind's table and the state of charge beside them exactly what the run without the series gives;
    chains faulted at construction add nothing, rows after a chain's fault exclude it."""
    g, t = a_fl(kind), a60_gpu()
    want, end = a_want(kind)
    steps, first = a_has_teeth(t["pv"], t["cov"], g["status"])
    assert g["variants"] == [_code(kind)] * len(A_WINDOWS) and _code(kind) & 15 == (14 if kind == "dispatch" else 15)
    assert g["guards"] == [0] * len(A_WINDOWS)
    _columns_equal(g["fleet"], want)
    plain = _a_table(kind)
    np.testing.assert_array_equal(g["raw"], plain["raw"])
    np.testing.assert_array_equal(g["soc"], plain["soc"])
    np.testing.assert_array_equal(g["soc"], end)
    fl = g["fleet"]
    dead = g["status"] == 1
    live = np.array([(~dead[:GC]).sum(), (~dead[GC:]).sum()])
    assert dead[:GC].any() and dead[GC:].any()
    np.testing.assert_array_equal(fl[:, 0, 2], live)                       # chains dead at construction add nothing
    faults = np.sort(np.argmax(t["cov"] == 255, axis=0)[(t["cov"][-1] == 255) & ~dead])
    assert len(faults) >= 3 and list(faults) == list(steps)
    n_ok = fl[..., 2].sum(axis=0)
    for k, s in enumerate(faults):                                          # rows after a chain's fault exclude it
        assert n_ok[s - 1] == live.sum() - k and n_ok[s] < n_ok[s - 1]
    assert n_ok[-1] == live.sum() - len(faults)
    par = D_PARAMS if kind == "dispatch" else S_PARAMS
    _row_identities(fl, [par[0, :GC].sum(), par[0, GC:].sum()])
    for k in range(13):                                                     # the rows summed per interval: the table over the chains
        rows = fl[:, k * IV:(k + 1) * IV].sum(axis=1)
        for col, tcol in ((4, 4), (5, 5), (7, 6), (8, 10)):
            assert [int(v) for v in rows[:, col]] == [int(g["raw"][k, tcol, :GC].sum()), int(g["raw"][k, tcol, GC:].sum())]
    one = fl.sum(axis=0)                                                    # the teeth (test_dispatch_fleet_cpu)
    assert int((one[:, 8] > 0).sum()) >= 2000
    night = one[:, 0] == 0
    assert night[:first].all() and not one[night, 5].any() and not one[night, 8].any()
    if kind == "schedule":                                                  # grid buying, at night too
        assert int((one[:, 4] > one[:, 1] + np.abs(one[:, 0])).sum()) >= 1000 and int((one[night, 7] > 0).sum()) >= 100
    else:
        assert not one[night, 7].any()


@pytest.mark.parametrize("kind", KINDS)
def test_pipelined_windows_same_bits(kind):
    """run(A_STEPS, window=4000): three windows through the pipeline (walks ahead of the expansions) give the bits of
    one tmh_run per window."""
    want, end = a_want(kind)
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, kind, A_STEPS, IV)
    fl = sim.enable_dispatch_fleet(A_STEPS, group_chains=GC)
    sim.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    assert _last(sim) == _code(kind)
    _columns_equal(_np(fl), want)
    np.testing.assert_array_equal(_np(raw), _a_table(kind)["raw"])
    np.testing.assert_array_equal(_np(sim.soc), end)


@pytest.mark.parametrize("kind,interval_s", [("dispatch", 128), ("schedule", 7), ("schedule", 128)])
@pytest.mark.parametrize("n,gc", [(1300, GC), (64, 0)])
def test_fleet_shapes(kind, interval_s, n, gc):
    """701 steps from 06:58 across sunrise: three groups with a partial last one of 276 chains and a partial
    wavefront, and a single wavefront in one group; night and daylight rows.  The schedule at interval_s 7 with
    c_rules: rule changes inside four-second groups and on both sides of the mid-tile flush (the 64th second of a
    128-second tile), every tile split into some nineteen pieces; at 128: one change per tile."""
    steps = 701
    pv, meter, cov = (a[:steps] for a in c60_traces(n))
    util = dispatch_util if kind == "dispatch" else schedule_util
    par, soc0 = util.tiled(n, "C")
    rules = schedule_util.c_rules(-(-steps // interval_s))
    assert kind == "dispatch" or len(set(np.diff(rules.astype(int)).tolist())) > 1
    want, end = _ref(kind, pv, meter, cov, interval_s, par, soc0, rules, gc=gc)
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, kind, steps, interval_s, par, soc0, rules)
    fl = sim.enable_dispatch_fleet(steps, group_chains=gc)
    assert tuple(fl.shape) == (3 if gc else 1, steps, 9) == want.shape
    sim.run(steps, trace=(), window=steps)
    assert _last(sim) == _code(kind)
    torch.cuda.synchronize()
    got = _np(fl)
    _columns_equal(got, want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    plain = _sim(n, C_START, **_kw60(C_STEPS))                              # the kind's existing kernels: the table beside
    rawp = _enable(plain, kind, steps, interval_s, par, soc0, rules)
    plain.run(steps, trace=(), window=steps)
    torch.cuda.synchronize()
    assert _last(plain) & 15 == (11 if kind == "dispatch" else 13)
    assert torch.equal(raw, rawp) and torch.equal(sim.soc, plain.soc)
    day = got[..., 0].sum(axis=0) != 0
    assert not day[:120].any() and day[-60:].all()                          # night and daylight rows
    assert got[-1, :, 2].max() <= (n - 1) % (gc or n) + 1 and got[-1].any()
    assert int(got[:, 0, 2].sum()) == n - int((cov[0] == 255).sum())
    if n > 1000:
        assert (cov[0] == 255).any() and int(got[..., 8].sum()) > 0        # construction faults; the limit binds
    _row_identities(got)


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_rule_is_the_battery_fleet_series(kind):
    """Tc = Td = 0 and L = none (the schedule: one such rule, G = 0): columns 0-7 are an enable_battery_fleet run's of
    the same batteries (the battery kind's OUT_FLEET kernel as the reference) and column 8 is 0."""
    from test_gpu_battery_fleet import a_fl as battery_fl
    greedy = np.vstack([D_PARAMS[:6], np.zeros((2, A_N), np.int64), np.full((1, A_N), 1 << 27, np.int64)])
    par = greedy if kind == "dispatch" else np.vstack([greedy, np.zeros((1, A_N), np.int64)])
    sim = _sim(A_N, A_START, **_kw60())
    _enable(sim, kind, A_STEPS, IV, par, D_SOC0, np.zeros(13, np.uint8))
    fl = sim.enable_dispatch_fleet(A_STEPS, group_chains=GC)
    _run_windows(sim, A_WINDOWS)
    want = battery_fl()
    got = _np(fl)
    np.testing.assert_array_equal(got[..., :8], want["fleet"])
    np.testing.assert_array_equal(_np(sim.soc), want["soc"])
    assert not got[..., 8].any() and int(got[..., 5].sum()) > 0


@pytest.mark.parametrize("case", ["one_rule", "equal_rules", "one_rule_throughout"])
def test_schedule_fleet_reduces_to_the_dispatch_fleet(case):
    """R = 1; R = 4 with all of a chain's rules equal; and an array that names rule 0 throughout: the dispatch fleet
    series of an enable_dispatch sim of the same households (rule 0), the other instantiation as the reference."""
    from tmhpvsim_amd import schedule
    R = schedule_util.R
    steps = 7300                                                            # into daylight, past eight interval edges
    dp = _sim(A_N, A_START, **_kw60())
    _enable(dp, "dispatch", A_STEPS, IV, schedule.to_dispatch_params(S_PARAMS, 0), S_SOC0)
    want = dp.enable_dispatch_fleet(steps, group_chains=GC)
    dp.run(steps, trace=(), window=3700)
    par, rules = {"one_rule": (S_PARAMS[:10], np.zeros(13, np.uint8)),
                  "equal_rules": (np.vstack([S_PARAMS[:6]] + [S_PARAMS[6:10]] * R), A_RULES),
                  "one_rule_throughout": (S_PARAMS, np.zeros(13, np.uint8))}[case]
    sim = _sim(A_N, A_START, **_kw60())
    _enable(sim, "schedule", A_STEPS, IV, par, S_SOC0, rules)
    fl = sim.enable_dispatch_fleet(steps, group_chains=GC)
    sim.run(steps, trace=(), window=3700)
    torch.cuda.synchronize()
    assert _last(dp) == _code("dispatch") and _last(sim) == _code("schedule")
    assert torch.equal(fl, want) and torch.equal(sim.soc, dp.soc)
    assert int(want[..., 8].sum()) > 0 and int(want[..., 7].sum()) > 0


def test_no_battery_gives_the_registers_per_second():
    """C = 0, ec = 2^16 and L = none: columns 4 and 5 are the import / export registers' per-second sums over the
    chains, from the traces; nothing is stored, charged or curtailed."""
    from tmhpvsim_amd import battery
    t = a60_gpu()
    par = D_PARAMS.copy()
    par[0], par[3], par[8] = 0, 1 << 16, 1 << 27
    sim = _sim(A_N, A_START, **_kw60())
    _enable(sim, "dispatch", A_STEPS, IV, par, np.zeros(A_N, np.int64))
    fl = sim.enable_dispatch_fleet(A_STEPS, group_chains=GC)
    _run_windows(sim, A_WINDOWS)
    ok, d = battery._ok_d(t["pv"], t["meter"], t["cov"])
    im, ex = np.where(ok, np.maximum(-d, 0), 0), np.where(ok, np.maximum(d, 0), 0)
    got = _np(fl)
    np.testing.assert_array_equal(got[..., 4], np.stack([im[:, :GC].sum(axis=1), im[:, GC:].sum(axis=1)]))
    np.testing.assert_array_equal(got[..., 5], np.stack([ex[:, :GC].sum(axis=1), ex[:, GC:].sum(axis=1)]))
    assert not got[..., 6:].any() and int(got[..., 4].sum()) > 0 and int(got[..., 5].sum()) > 0


@pytest.mark.parametrize("start,full_pairs", [("2019-09-05 02:00:00", 4000), ("2019-09-05 12:30:00", 2000)])
def test_range_ends_of_the_grid_rule(start, full_pairs):
    """The ends of the ranges a grid-charging rule reaches: 512 chains x 300 s under one rule Tc = Td = 2^27 (hold),
    G = 2^27, Pc = 2^27, C = 2^40 - 1, soc0 = 0 -- every ok chain-second charges exactly 2^27 (the battery cannot
    fill within 300 s) and imports 2^27 - d.  A half-wave of 32 ok lanes therefore sums its charge to exactly 2^32,
    one more than a 32-bit partial holds, and at night (d <= 0) its import to 2^32 or more: a kernel with 32-bit
    half-wave partials fails columns 4 and 7 of both runs.  At 02:00 no chain is dead and all 4,800 (second,
    half-wave) pairs are full (the night path); at 12:30 twelve chains are dead and 2,400 pairs are full (the daylight
    path).  The conditions are asserted of a separate sim's traces."""
    from tmhpvsim_amd import battery
    n, steps = 512, 300
    kw = dict(prec=PREC, chain0=A_CHAIN0, mp=modules_params(), horizon=steps)
    tr = _sim(n, start, **kw)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    pv, meter, cov = (_np(out[k]) for k in ("pv", "meter", "covered"))
    top = 1 << 27
    par = np.zeros((10, n), dtype=np.int64)
    par[0], par[1], par[3:5] = (1 << 40) - 1, top, 1 << 16
    par[6:10] = top                                                         # Tc, Td (hold), L (none), G
    rules = np.zeros(1, np.uint8)
    want, end = _ref("schedule", pv, meter, cov, steps, par, 0, rules)
    ok, d = battery._ok_d(pv, meter, cov)
    full = ok.reshape(steps, n // 32, 32).all(axis=2)                       # (second, half-wave) pairs of 32 ok lanes
    dsum = np.where(ok, d, 0).reshape(steps, n // 32, 32).sum(axis=2)
    night = start.endswith("02:00:00")
    pairs = int((full & (dsum <= 0)).sum()) if night else int(full.sum())   # charge sum 2^32 (and import sum >= 2^32)
    print("full pairs", int(full.sum()), "with import >= 2^32", int((full & (dsum <= 0)).sum()), "dead", int((cov[0] == 255).sum()))
    assert pairs >= full_pairs
    np.testing.assert_array_equal(want[0, :, 7], want[0, :, 2] << 27)       # every ok chain-second charges 2^27
    np.testing.assert_array_equal(want[0, :, 4], (want[0, :, 2] << 27) - np.where(ok, d, 0).sum(axis=1))
    assert night == (not np.nan_to_num(pv).any()) and (night or (cov[0] == 255).any())
    sim = _sim(n, start, **kw)
    _enable(sim, "schedule", steps, steps, par, np.zeros(n, np.int64), rules)
    fl = sim.enable_dispatch_fleet(steps, group_chains=GC)
    sim.run(steps, trace=(), window=steps)
    torch.cuda.synchronize()
    assert _last(sim) == _code("schedule")
    _columns_equal(_np(fl), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    assert int(end.max()) == steps << 27 and not want[..., 5].any() and not want[..., 8].any()


def test_corner_recipe_behind_dispatch():
    """range_util.corners on input A: every parameter of every chain at an end of its range (C up to 2^40 - 1, powers,
    thresholds and limits 0 and 2^27, efficiencies 2^15 and 2^16), the state of charge starting at an end of [0, C]."""
    t = a60_gpu()
    par, soc0 = corners()
    want, end = _ref("dispatch", t["pv"], t["meter"], t["cov"], params=par, soc0=soc0)
    sim = _sim(A_N, A_START, **_kw60())
    _enable(sim, "dispatch", A_STEPS, IV, par, soc0)
    fl = sim.enable_dispatch_fleet(A_STEPS, group_chains=GC)
    _run_windows(sim, A_WINDOWS)
    _columns_equal(_np(fl), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    assert int(want[..., 6].max()) > 1 << 40 and int(want[..., 8].sum()) > 0   # (a group's stored energy: above one chain's range)
    _row_identities(_np(fl), [par[0, :GC].sum(), par[0, GC:].sum()])


def test_two_sims_add_into_one_buffer():
    """Chains [5000, 5512) and [5512, 6000) as two sims adding into one one-group buffer: the sum of the two
    references, which is the whole batch's one-group table."""
    t = a60_gpu()
    want, _ = a_want("dispatch")
    steps = 7000
    buf = torch.zeros(1, steps, 9, dtype=torch.int64, device="cuda:0")
    refs = []
    for a, b in ((0, GC), (GC, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        _enable(s, "dispatch", A_STEPS, IV, D_PARAMS[:, a:b], D_SOC0[a:b])
        assert s.enable_dispatch_fleet(steps, buffer=buf) is buf
        s.run(steps, trace=())
        refs.append(_ref("dispatch", t["pv"][:steps, a:b], t["meter"][:steps, a:b], t["cov"][:steps, a:b],
                         params=D_PARAMS[:, a:b], soc0=D_SOC0[a:b], gc=0)[0])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(buf), refs[0] + refs[1])
    np.testing.assert_array_equal(_np(buf)[0], want[:, :steps].sum(axis=0))
    assert int(_np(buf)[..., 8].sum()) > 0
    with pytest.raises(ValueError, match="dispatch fleet buffer"):
        s.enable_dispatch_fleet(steps, buffer=buf[:, :, :8])
    with pytest.raises(ValueError, match="dispatch fleet buffer"):
        s.enable_dispatch_fleet(steps + 1, buffer=buf)


@pytest.mark.parametrize("kind", KINDS)
def test_statistics_and_table_unperturbed_by_the_fleet(kind):
    """The histogram and the per-chain totals with the series on are the kind-only sim's and a statistics-only sim's,
    bit for bit; the table and the state of charge are the kind-only sim's."""
    from test_gpu_trace3 import HISTS
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw60(steps)
    par, soc0 = (D_PARAMS, D_SOC0) if kind == "dispatch" else (S_PARAMS, S_SOC0)
    par, soc0, rules = par[:, :n], soc0[:n], A_RULES[:3]
    both, alone, stats = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    for s in (both, alone, stats):
        s.enable_stats(**HISTS["default"])
    ra, rb = _enable(both, kind, steps, 600, par, soc0, rules), _enable(alone, kind, steps, 600, par, soc0, rules)
    fl = both.enable_dispatch_fleet(steps, group_chains=GC)
    for s in (both, alone, stats):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) == _code(kind) and _last(alone) & 15 == (11 if kind == "dispatch" else 13)
    for other in (alone, stats):
        assert torch.equal(both.hist, other.hist)
        assert torch.equal(both.chain_acc.view(torch.int64), other.chain_acc.view(torch.int64))
    assert int(both.hist.sum()) == int(fl[..., 2].sum()) == int(ra[:, 2].sum()) > 0
    assert torch.equal(ra, rb) and torch.equal(both.soc, alone.soc)
    assert int(fl[..., 7].sum()) == int(ra[:, 6].sum()) > 0 and int(fl[..., 4].sum()) == int(ra[:, 4].sum()) > 0
    assert int(fl[..., 8].sum()) == int(ra[:, 10].sum()) and int(fl[..., 5].sum()) == int(ra[:, 5].sum()) > 0
    _row_identities(_np(fl))


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "dispatch fleet series" before anything is launched:
    the chains' state and the batteries' stay as they were, the tables and the rows all zeros; the sim runs
    afterwards.  What was refused without the series stays refused in the same words."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.params import site_grid
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, soc0 = D_PARAMS[:, :n], D_SOC0[:n]
    spar, ssoc0, rules = S_PARAMS[:, :n], S_SOC0[:n], np.zeros(9, np.uint8)
    rows = torch.zeros(2, 500, 9, dtype=torch.int64, device="cuda:0")
    fleet = _lib.Series(rows.data_ptr(), 0, 500, GC, 2, 0)

    def refused(sim, match, word="dispatch fleet series", step0=0, k=100):
        before = sim.state.clone()
        soc = sim.soc.clone() if sim.soc is not None else None
        ws = sim.workspace(k)
        tr = _lib.Trace(None, None, None, None, None, sim.n)
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, None, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg and word in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, None, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        assert match in L.tmh_last_error().decode()
        assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                          ws.numel() - pb, None) == -1
        assert match in L.tmh_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and not bool(rows.any())
        if soc is not None:
            assert torch.equal(soc, sim.soc)
        for raw in (sim.dispatch_raw, sim.schedule_raw, sim.battery_raw, sim.storage_raw, sim.intervals_raw):
            assert raw is None or not bool(raw.any())

    # the setter: tmh_set_battery_fleet's bad-struct cases in its own words, and an fp32 engine
    sim = _sim(n, start, prec=PREC, horizon=1000)
    p = rows.data_ptr()
    for args, word in (((None, 0, 500, GC, 2, 0), b"buffer"), ((p, 0, 0, GC, 2, 0), b"n_steps"), ((p, 0, 500, GC, 0, 0), b"n_groups"),
                       ((p + 4, 0, 500, GC, 2, 0), b"8-byte aligned"), ((p, 0, 500, 100, 6, 0), b"multiple of 512"),
                       ((p, 0, 500, 0, 2, 0), b"multiple of 512")):
        assert L.tmh_set_dispatch_fleet(sim._eng, C.byref(_lib.Series(*args))) == -1
        assert word in L.tmh_last_error() and b"dispatch fleet series" in L.tmh_last_error()
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    assert L.tmh_set_dispatch_fleet(f32._eng, C.byref(fleet)) == -1
    assert b"fp64" in L.tmh_last_error() and b"dispatch fleet series" in L.tmh_last_error()
    assert L.tmh_set_dispatch_fleet(f32._eng, None) == 0
    # neither dispatch nor the schedule: set alone, and left behind when the kind is switched off
    with pytest.raises(ValueError, match="enable_dispatch or enable_schedule first"):
        sim.enable_dispatch_fleet(500)
    _lib.check(L.tmh_set_dispatch_fleet(sim._eng, C.byref(fleet)))
    refused(sim, "needs battery dispatch or the schedule")
    _enable(sim, "dispatch", 500, 60, par, soc0)
    _lib.check(L.tmh_set_dispatch(sim._eng, None))
    refused(sim, "needs battery dispatch or the schedule")
    sim.enable_dispatch(None)
    # any other kind: the battery kind, storage, interval metering, the sweeps; two kinds
    from test_gpu_battery import _enable as battery_enable
    battery_enable(sim, 500, 60, par[:6], soc0)
    refused(sim, "cannot run beside the battery kind")
    sim.enable_battery(None)
    sim.enable_intervals(500, 60)
    refused(sim, "cannot run beside interval metering")
    sim.enable_intervals(None)
    sim.enable_dispatch_sweep(500, 60, params=_dev(np.stack([par, par])), soc=_dev(np.stack([soc0, soc0])))
    refused(sim, "cannot run beside the dispatch sweep")
    sim.enable_dispatch_sweep(None)
    _enable(sim, "dispatch", 500, 60, par, soc0)
    tab2, par2, soc2, rul2 = torch.zeros(9, 13, n, dtype=torch.int64, device="cuda:0"), _dev(spar), _dev(ssoc0), _dev(rules)
    work2 = torch.empty(L.tmh_storage_work_bytes(n, 500), dtype=torch.uint8, device="cuda:0")
    sc = _lib.Schedule(_lib.Intervals(tab2.data_ptr(), 0, 500, 60, n), soc2.data_ptr(), work2.data_ptr(), work2.numel(),
                       par2.data_ptr(), rul2.data_ptr(), 4)
    _lib.check(L.tmh_set_schedule(sim._eng, C.byref(sc)))                   # (a C caller: the sim refuses the second kind itself)
    refused(sim, "two table kinds")
    _lib.check(L.tmh_set_schedule(sim._eng, None))
    assert not bool(tab2.any())
    # tmh_set_series or tmh_set_battery_fleet set too
    ser = sim.enable_series(500)
    refused(sim, "tmh_set_series")
    assert not bool(ser.any())
    sim.enable_series(None)
    old = torch.zeros(2, 500, 8, dtype=torch.int64, device="cuda:0")
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(_lib.Series(old.data_ptr(), 0, 500, GC, 2, 0))))
    refused(sim, "tmh_set_battery_fleet")
    # ... and without the series the old refusal of the battery fleet series beside dispatch, in its words
    _lib.check(L.tmh_set_dispatch_fleet(sim._eng, None))
    refused(sim, "battery dispatch and a battery fleet series are both set: the fleet series is the battery kind's",
            word="battery fleet series")
    _lib.check(L.tmh_set_battery_fleet(sim._eng, None))
    assert not bool(old.any())
    with pytest.raises(ValueError, match="battery fleet series is enabled|call enable_battery first"):
        sim.enable_battery_fleet(500)
    # compacted windows
    _lib.check(L.tmh_set_dispatch_fleet(sim._eng, C.byref(fleet)))
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    _lib.check(L.tmh_set_chain_ids(sim._eng, C.c_void_p(ids.data_ptr()), n))
    refused(sim, "compacted chains")
    _lib.check(L.tmh_set_chain_ids(sim._eng, None, 0))
    assert sim.enable_dispatch_fleet(500, group_chains=GC, buffer=rows) is rows
    with pytest.raises(ValueError, match="dispatch fleet series cannot run compacted"):
        sim.run(200, trace=(), window=100, compact=True)
    # the window and the groups
    sim.enable_dispatch_fleet(400, group_chains=GC)                        # (inside the table's 500 steps, so the
    refused(sim, "outside the dispatch fleet series", step0=350, k=100)    #  kind's own window check passes)
    sim.enable_dispatch_fleet(490, step0=10, group_chains=GC)
    refused(sim, "outside the dispatch fleet series", step0=0, k=100)
    with pytest.raises(ValueError, match="outside the dispatch fleet series"):
        sim.run(100, trace=())
    _lib.check(L.tmh_set_dispatch_fleet(sim._eng, C.byref(_lib.Series(p, 0, 500, GC, 1, 0))))
    refused(sim, "1 groups x 512 chains < n_chains 600")
    with pytest.raises(ValueError, match="multiple of 512"):
        sim.enable_dispatch_fleet(500, group_chains=100)
    # per-chain sites (dispatch runs with them; its fleet series does not)
    st = _sim(n, start, prec=PREC, horizon=1000, sites=site_grid(30, 20))
    _enable(st, "dispatch", 500, 60, par, soc0)
    with pytest.raises(ValueError, match="per-chain sites"):
        st.enable_dispatch_fleet(500, group_chains=GC, buffer=rows)
    _lib.check(L.tmh_set_dispatch_fleet(st._eng, C.byref(fleet)))
    refused(st, "per-chain sites")
    # traces stay refused in the kind's words; the sim has not moved
    sim.enable_dispatch_fleet(500, step0=0, group_chains=GC, buffer=rows)
    with pytest.raises(ValueError, match="trace"):
        sim.run(100, trace=("pv",))
    assert sim.step == 0
    # switched off and on again, the sim runs: rows only while it is on
    sim.enable_dispatch_fleet(None)
    assert sim.dispatch_fleet_raw is None
    sim.run(100, trace=())
    assert _last(sim) == _lib.OUT_DISPATCH | _lib.OUT_FP64
    torch.cuda.synchronize()
    ok1 = int(sim.dispatch_raw[:, 2].sum())
    assert not bool(rows.any()) and ok1 > 0
    sim.enable_dispatch_fleet(500, step0=0, group_chains=GC, buffer=rows)
    sim.run(100, trace=())
    assert _last(sim) == _code("dispatch")
    torch.cuda.synchronize()
    got = _np(rows)
    assert not got[:, :100].any() and not got[:, 200:].any() and got[0, 100:200, 2].min() > 0 and got[1, 100:200, 2].min() > 0
    assert int(got[..., 2].sum()) == int(sim.dispatch_raw[:, 2].sum()) - ok1   # (the rows of the second run only)
    _row_identities(got)
    sim.enable_dispatch(None)                                               # the kind off: its fleet series with it
    assert sim.dispatch_fleet_raw is None and sim.dispatch_raw is None
    _enable(sim, "schedule", 500, 60, spar, ssoc0, rules, step0=200)        # and behind the schedule, the same sim
    sim.enable_dispatch_fleet(300, step0=200, group_chains=GC)
    sim.run(100, trace=())
    assert _last(sim) == _code("schedule")
    sim.enable_schedule(None)
    assert sim.dispatch_fleet_raw is None and sim.schedule_raw is None
