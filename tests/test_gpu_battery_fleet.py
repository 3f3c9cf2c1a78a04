"""The battery fleet series on the GPU (tmh_set_battery_fleet, BatchedSim.enable_battery_fleet; fp64 throughout):
integers, so every comparison with the traces' table (battery.fleet_from_traces, a plain loop over the seconds) is
bit for bit.  The expected rows always come from traces of separate sims of the same chains (test_gpu_storage.
a60_gpu / c60_traces: computed once, shared with the storage and battery tests), never from the kernels under
test.  The batteries are battery_util.recipe's."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from battery_util import recipe, uniform
from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_WINDOWS, a_has_teeth
from storage_util import A_BATTERY, modules_params
from storage_util import battery as storage_battery
from test_gpu_battery import _enable, _identities, a_want
from test_gpu_registers import C_START, C_STEPS, _run_windows
from test_gpu_series import _last, _np, _sim
from test_gpu_storage import IV, PREC, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARAMS, SOC0 = recipe()
GC = 512


def _row_identities(raw, cap_sum=None):
    """Columns 4-7 >= 0, the discharging power [7] - sum of b >= 0 with sum of b from [4] - [5] == [1] - [0] + sum of
    b, the counts consistent, and [6] <= the sum of the capacities."""
    assert (raw[..., 4:] >= 0).all() and (raw[..., 2] >= raw[..., 3]).all() and (raw[..., 3] >= 0).all()
    sb = raw[..., 4] - raw[..., 5] - (raw[..., 1] - raw[..., 0])
    assert (raw[..., 7] - sb >= 0).all()
    assert (raw[..., 4] <= raw[..., 1] + np.abs(raw[..., 0])).all() and (raw[..., 5] <= np.abs(raw[..., 0])).all()
    if cap_sum is not None:
        assert (raw[..., 6].T <= np.asarray(cap_sum)).all()


@functools.lru_cache(maxsize=None)
def a_fleet_want():
    """The expected rows of input A in groups of 512 and the end state, from the storage tests' traces."""
    from tmhpvsim_amd import battery
    t = a60_gpu()
    want, end = battery.fleet_from_traces(t["pv"], t["meter"], t["cov"], params=PARAMS, soc0=SOC0, group_chains=GC)
    want.setflags(write=False)
    return want, end


@functools.lru_cache(maxsize=None)
def a_fl():
    """The battery sim of input A with its fleet series, one tmh_run per window of A_WINDOWS."""
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, A_STEPS, IV)
    fl = sim.enable_battery_fleet(A_STEPS, group_chains=GC)
    assert fl is sim.battery_fleet_raw and tuple(fl.shape) == (2, A_STEPS, 8) and fl.dtype == torch.int64
    variants, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), fleet=_np(fl), soc=_np(sim.soc), variants=variants, guards=guards, status=sim.status())


def test_fleet_equals_the_traces_rows():
    """The main test: all eight columns of both groups (512 chains and a partial group of 488) bit for bit over
    two windows (the second off the four-step grid), the battery table and the state of charge beside them as
    without a fleet series; chains faulted at construction add nothing, rows after a chain's fault exclude it."""
    from tmhpvsim_amd import _lib
    g, t = a_fl(), a60_gpu()
    want, end = a_fleet_want()
    steps, first = a_has_teeth(t["pv"], t["cov"], g["status"])
    assert g["variants"] == [_lib.OUT_BATTERY_FLEET | _lib.OUT_FP64] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    differ = [int((g["fleet"][..., col] != want[..., col]).sum()) for col in range(8)]   # (group, second) rows per column
    print("rows that differ per column", differ, "of", 2 * A_STEPS)
    assert differ == [0] * 8
    table, tend = a_want()
    np.testing.assert_array_equal(g["raw"], table)
    np.testing.assert_array_equal(g["soc"], end)
    np.testing.assert_array_equal(g["soc"], tend)
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
    _row_identities(fl, [PARAMS[0, :GC].sum(), PARAMS[0, GC:].sum()])
    night = fl[..., 0].sum(axis=0) == 0
    assert night[:first].all() and not night[-3600:].any()
    assert (fl[..., 7].sum(axis=0)[night] == 0).all() and (fl[..., 5].sum(axis=0)[night] == 0).all()
    one = fl.sum(axis=0)                                                    # the teeth (test_battery_fleet_cpu)
    assert int(((one[:, 4] > 0) & (one[:, 5] > 0)).sum()) >= 2000
    d6 = np.diff(one[:, 6])
    assert int((d6 > 0).sum()) >= 1000 and int((d6 < 0).sum()) >= 1000


def test_pipelined_windows_same_bits():
    """run(A_STEPS, window=4000): three windows through the pipeline (walks ahead of the expansions) give the
    bits of one tmh_run per window."""
    want, end = a_fleet_want()
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV)
    fl = sim.enable_battery_fleet(A_STEPS, group_chains=GC)
    sim.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(fl), want)
    np.testing.assert_array_equal(_np(fl), a_fl()["fleet"])
    np.testing.assert_array_equal(_np(raw), a_want()[0])
    np.testing.assert_array_equal(_np(sim.soc), end)


@pytest.mark.parametrize("n,gc", [(1300, GC), (64, 0)])
def test_fleet_shapes(n, gc):
    """701 steps from 06:58 across sunrise: three groups with a partial last one of 276 chains and a partial
    wavefront, and a single wavefront in one group; night and daylight rows."""
    from tmhpvsim_amd import _lib, battery
    steps = 701
    pv, meter, cov = (a[:steps] for a in c60_traces(n))
    reps = -(-n // A_N)
    par, soc0 = np.tile(PARAMS, (1, reps))[:, :n], np.tile(SOC0, reps)[:n]
    want, end = battery.fleet_from_traces(pv, meter, cov, params=par, soc0=soc0, group_chains=gc)
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, steps, 128, par, soc0)
    fl = sim.enable_battery_fleet(steps, group_chains=gc)
    assert tuple(fl.shape) == (3 if gc else 1, steps, 8) == want.shape
    sim.run(steps, trace=(), window=steps)
    assert _last(sim) == _lib.OUT_BATTERY_FLEET | _lib.OUT_FP64
    torch.cuda.synchronize()
    got = _np(fl)
    for col in range(8):
        np.testing.assert_array_equal(got[..., col], want[..., col], err_msg=f"column {col}")
    np.testing.assert_array_equal(_np(sim.soc), end)
    table, tend = battery.from_traces(pv, meter, cov, 128, params=par, soc0=soc0)
    np.testing.assert_array_equal(_np(raw), table)
    np.testing.assert_array_equal(tend, end)
    day = got[..., 0].sum(axis=0) != 0
    assert not day[:120].any() and day[-60:].all()                          # night and daylight rows
    assert got[-1, :, 2].max() <= (n - 1) % (gc or n) + 1 and got[-1].any()
    assert int(got[:, 0, 2].sum()) == n - int((cov[0] == 255).sum())
    if n > 1000:
        assert (cov[0] == 255).any()                                        # construction faults
    _row_identities(got)


def test_fleet_per_chain_sites():
    """The per-chain-sites replay kernel, test_battery_per_chain_sites' setting."""
    import dataclasses
    from tmhpvsim_amd import _lib, battery
    from tmhpvsim_amd.params import ModelParams, site_grid
    n, steps, start = 512, 3000, "2019-06-21 04:45:00"
    sites = site_grid(32, 16)
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    mp = dataclasses.replace(modules_params(), cc_mode=ModelParams().cc_mode, seed=0x51E)
    sim = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    raw = _enable(sim, steps + 1, 450, par, soc0, step0=-1)
    fl = sim.enable_battery_fleet(steps, group_chains=GC)
    sim.run(steps, trace=(), window=1700)
    assert _last(sim) == _lib.OUT_BATTERY_FLEET | _lib.OUT_SITES | _lib.OUT_FP64
    tr = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    want, end = battery.fleet_from_traces(out["pv"], out["meter"], out["covered"], params=par, soc0=soc0, group_chains=GC)
    got = _np(fl)
    for col in range(8):
        np.testing.assert_array_equal(got[..., col], want[..., col], err_msg=f"column {col}")
    np.testing.assert_array_equal(_np(sim.soc), end)
    table, _ = battery.from_traces(out["pv"], out["meter"], out["covered"], 450, origin=1, params=par, soc0=soc0)
    np.testing.assert_array_equal(_np(raw), table)
    assert all(int(want[..., c].sum()) > 0 for c in range(8))
    _row_identities(got)


def test_two_sims_add_into_one_buffer():
    """Chains [5000, 5512) and [5512, 6000) as two sims adding into one one-group buffer: the sum of the two
    references, which is the whole batch's one-group table."""
    from tmhpvsim_amd import battery
    t = a60_gpu()
    want, _ = a_fleet_want()
    steps = 6200                                                            # into the first minutes of daylight
    buf = torch.zeros(1, steps, 8, dtype=torch.int64, device="cuda:0")
    refs = []
    for a, b in ((0, GC), (GC, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        _enable(s, A_STEPS, IV, PARAMS[:, a:b], SOC0[a:b])
        assert s.enable_battery_fleet(steps, buffer=buf) is buf
        s.run(steps, trace=())
        refs.append(battery.fleet_from_traces(t["pv"][:steps, a:b], t["meter"][:steps, a:b], t["cov"][:steps, a:b],
                                              params=PARAMS[:, a:b], soc0=SOC0[a:b])[0])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(buf), refs[0] + refs[1])
    np.testing.assert_array_equal(_np(buf)[0], want[:, :steps].sum(axis=0))
    with pytest.raises(ValueError, match="battery fleet buffer"):
        s.enable_battery_fleet(steps, buffer=buf[:, :, :4])
    with pytest.raises(ValueError, match="battery fleet buffer"):
        s.enable_battery_fleet(steps + 1, buffer=buf)
    with pytest.raises(ValueError, match="battery fleet buffer"):
        s.enable_battery_fleet(steps, group_chains=GC, buffer=torch.zeros(0, steps, 8, dtype=torch.int64, device="cuda:0"))


def test_lossless_rows_follow_storage():
    """Efficiencies 1, no standby drain, one battery for all: columns 4-7 follow storage's per-second rule --
    fleet_from_traces with those parameters, whose interval sums and end state are storage.from_traces' (the
    storage tests' expected table)."""
    from tmhpvsim_amd import _lib, battery
    t = a60_gpu()
    bat = storage_battery(A_BATTERY)
    par = uniform(A_N, bat["capacity"], bat["p_charge"], bat["p_discharge"])
    want, end = battery.fleet_from_traces(t["pv"], t["meter"], t["cov"], params=par, soc0=bat["soc0"])
    st = t["want"]                                                          # storage.from_traces' table
    np.testing.assert_array_equal(end, t["end"])
    for k in range(st.shape[0]):
        rows = want[0, k * IV:(k + 1) * IV]
        assert [int(rows[:, c].sum()) for c in (4, 5, 7)] == [int(st[k, c].sum()) for c in (4, 5, 6)]
    sim = _sim(A_N, A_START, **_kw60())
    raw = sim.enable_battery(A_STEPS, IV, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, **A_BATTERY)
    fl = sim.enable_battery_fleet(A_STEPS)
    _run_windows(sim, A_WINDOWS)
    assert _last(sim) == _lib.OUT_BATTERY_FLEET | _lib.OUT_FP64
    np.testing.assert_array_equal(_np(fl), want)
    np.testing.assert_array_equal(_np(raw)[:, :9], st)
    np.testing.assert_array_equal(_np(sim.soc), end)


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_statistics_and_table_unperturbed_by_the_fleet(spec):
    """The histogram and the per-chain totals with the fleet series on are a battery-only sim's and a
    statistics-only sim's, bit for bit; the battery table and the state of charge are the battery-only sim's."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw60(steps)
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    both, bat, stats = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    for s in (both, bat, stats):
        s.enable_stats(**HISTS[spec])
    ra, rb = _enable(both, steps, 600, par, soc0), _enable(bat, steps, 600, par, soc0)
    fl = both.enable_battery_fleet(steps, group_chains=GC)
    for s in (both, bat, stats):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) == _lib.OUT_BATTERY_FLEET | _lib.OUT_FP64 and _last(bat) == _lib.OUT_BATTERY | _lib.OUT_FP64
    assert _last(stats) & 7 == _lib.OUT_STATS
    for other in (bat, stats):
        assert torch.equal(both.hist, other.hist)
        assert torch.equal(both.chain_acc.view(torch.int64), other.chain_acc.view(torch.int64))
    assert int(both.hist.sum()) == int(fl[..., 2].sum()) == int(ra[:, 2].sum()) > 0
    assert torch.equal(ra, rb) and torch.equal(both.soc, bat.soc)
    assert int(fl[..., 7].sum()) == int(ra[:, 6].sum()) > 0 and int(fl[..., 4].sum()) == int(ra[:, 4].sum()) > 0
    _identities(_np(ra))
    _row_identities(_np(fl))


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "battery fleet" before anything is launched:
    the chains' state and the batteries' stay as they were, the table and the rows all zeros.  What was refused
    without a fleet series stays refused in the same words."""
    from tmhpvsim_amd import _lib
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    rows = torch.zeros(2, 500, 8, dtype=torch.int64, device="cuda:0")
    fleet = _lib.Series(rows.data_ptr(), 0, 500, GC, 2, 0)

    def refused(sim, match, word="battery fleet", step0=0, k=100):
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
        for raw in (sim.battery_raw, sim.storage_raw):
            assert raw is None or not bool(raw.any())

    # the setter: tmh_set_series' bad-struct cases in its own words, and an fp32 engine
    sim = _sim(n, start, prec=PREC, horizon=1000)
    p = rows.data_ptr()
    for args, word in (((None, 0, 500, GC, 2, 0), b"buffer"), ((p, 0, 0, GC, 2, 0), b"n_steps"), ((p, 0, 500, GC, 0, 0), b"n_groups"),
                       ((p + 4, 0, 500, GC, 2, 0), b"8-byte aligned"), ((p, 0, 500, 100, 6, 0), b"multiple of 512"),
                       ((p, 0, 500, 0, 2, 0), b"multiple of 512")):
        assert L.tmh_set_battery_fleet(sim._eng, C.byref(_lib.Series(*args))) == -1
        assert word in L.tmh_last_error() and b"battery fleet" in L.tmh_last_error()
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    assert L.tmh_set_battery_fleet(f32._eng, C.byref(fleet)) == -1
    assert b"fp64" in L.tmh_last_error() and b"battery fleet" in L.tmh_last_error()
    assert L.tmh_set_battery_fleet(f32._eng, None) == 0
    # a fleet series without the battery kind: set alone, and left behind when the kind is switched off
    with pytest.raises(ValueError, match="enable_battery first"):
        sim.enable_battery_fleet(500)
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(fleet)))
    refused(sim, "needs the battery kind")
    _enable(sim, 500, 60, par, soc0)
    _lib.check(L.tmh_set_battery(sim._eng, None))
    refused(sim, "needs the battery kind")
    # beside battery storage (the lossless kind), in either order
    _lib.check(L.tmh_set_battery_fleet(sim._eng, None))
    sim.enable_battery(None)
    sim.enable_storage(500, 60, **A_BATTERY)
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(fleet)))          # storage, then the fleet series
    refused(sim, "battery storage")
    sim.enable_storage(None)
    sim.enable_storage(500, 60, **A_BATTERY)                               # the fleet series, then storage
    refused(sim, "battery storage")
    sim.enable_storage(None)
    # compacted windows
    _enable(sim, 500, 60, par, soc0)
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    _lib.check(L.tmh_set_chain_ids(sim._eng, C.c_void_p(ids.data_ptr()), n))
    refused(sim, "compacted chains")
    _lib.check(L.tmh_set_chain_ids(sim._eng, None, 0))
    assert sim.enable_battery_fleet(500, group_chains=GC, buffer=rows) is rows
    with pytest.raises(ValueError, match="battery fleet series cannot run compacted"):
        sim.run(200, trace=(), window=100, compact=True)
    # the window and the groups
    sim.enable_battery_fleet(400, group_chains=GC)                         # (inside the table's 500 steps, so the
    refused(sim, "outside the battery fleet", step0=350, k=100)            #  battery kind's own window check passes)
    sim.enable_battery_fleet(490, step0=10, group_chains=GC)
    refused(sim, "outside the battery fleet", step0=0, k=100)
    with pytest.raises(ValueError, match="outside the battery fleet"):
        sim.run(100, trace=())
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(_lib.Series(p, 0, 500, GC, 1, 0))))
    refused(sim, "1 groups x 512 chains < n_chains 600")
    with pytest.raises(ValueError, match="multiple of 512"):
        sim.enable_battery_fleet(500, group_chains=100)
    # what the battery kind refuses stays refused in its words, a fleet series (tmh_set_series) beside it included
    sim.enable_battery_fleet(500, group_chains=GC, buffer=rows)
    ser = sim.enable_series(500)
    refused(sim, "battery tables and a fleet series are both set", word="battery")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    with pytest.raises(ValueError, match="trace"):
        sim.run(100, trace=("pv",))
    assert sim.step == 0
    # switched off and on again, the sim runs: rows only while it is on
    sim.enable_battery_fleet(None)
    assert sim.battery_fleet_raw is None
    sim.run(100, trace=())
    assert _last(sim) == _lib.OUT_BATTERY | _lib.OUT_FP64
    torch.cuda.synchronize()
    ok1 = int(sim.battery_raw[:, 2].sum())
    assert not bool(rows.any()) and ok1 > 0
    sim.enable_battery_fleet(500, step0=0, group_chains=GC, buffer=rows)
    sim.run(100, trace=())
    assert _last(sim) == _lib.OUT_BATTERY_FLEET | _lib.OUT_FP64
    torch.cuda.synchronize()
    got = _np(rows)
    assert not got[:, :100].any() and not got[:, 200:].any() and got[0, 100:200, 2].min() > 0 and got[1, 100:200, 2].min() > 0
    assert int(got[..., 2].sum()) == int(sim.battery_raw[:, 2].sum()) - ok1   # (the rows of the second run only)
    _row_identities(got)
    sim.enable_battery(None)                                                # the kind off: its fleet series with it
    assert sim.battery_fleet_raw is None and sim.battery_raw is None


def test_battery_cli_fleet(tmp_path):
    """`battery ... --fleet out.csv --bin 60`: the CSV is fleet_to_watts of the reference from a separate sim's
    traces; the command's other outputs are a run's without --fleet, byte for byte."""
    from click.testing import CliRunner
    from tmhpvsim_amd import battery
    from tmhpvsim_amd.cli import FLEET_CSV, main
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import ModelParams
    n, steps, start = 64, 701, "2019-09-06T12:00:00"
    args = ["--batch", str(n), "--seconds", str(steps), "--interval", "600", "--no-realtime", "--capacity-wh", "0.5,0,0.25",
            "--charge-w", "1000", "--discharge-w", "3000,1500", "--charge-eff", "0.95", "--discharge-eff", "0.9,1.0",
            "--standby-w", "2", "--soc0-wh", "0.25,0,0.25"]
    f, z, g = tmp_path / "bt.csv", tmp_path / "bt.npz", tmp_path / "fleet.csv"
    f0, z0 = tmp_path / "bt0.csv", tmp_path / "bt0.npz"
    r = CliRunner().invoke(main, ["battery", str(f), *args, "--all-chains", str(z), "--fleet", str(g), "--bin", "60"])
    assert r.exit_code == 0, r.output
    r = CliRunner().invoke(main, ["battery", str(f0), *args, "--all-chains", str(z0)])
    assert r.exit_code == 0, r.output
    assert open(f, "rb").read() == open(f0, "rb").read()
    a, b = np.load(z), np.load(z0)
    assert sorted(a.files) == sorted(b.files)
    for key in a.files:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    mp = ModelParams()
    deal = lambda vals: [vals[i % len(vals)] for i in range(n)]
    par = battery.quantize_params(deal([0.5, 0, 0.25]), 1000.0, deal([3000.0, 1500.0]), 0.95, deal([0.9, 1.0]), 2.0, n=n)
    soc0 = battery.quantize_soc(deal([0.25, 0, 0.25]), par)
    tr = BatchedSim(n, start, tz=mp.site.tz, params=ModelParams(seed=0x5EED), precision="fp64", device="cuda:0", horizon=steps)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    raw, _ = battery.fleet_from_traces(out["pv"], out["meter"], out["covered"], params=par, soc0=soc0)
    want = battery.fleet_to_watts(raw, bin_s=60, mean=True)
    rows = list(csv.reader(open(g)))
    assert rows[0] == ["time"] + [name for name, _ in FLEET_CSV] and len(rows) == 1 + 12
    assert [row[0] for row in rows[1:3]] == ["2019-09-06 12:00:00", "2019-09-06 12:01:00"]
    for k, row in enumerate(rows[1:]):
        assert [float(x) for x in row[1:]] == [float(want[key][0, k]) for _, key in FLEET_CSV], k
    assert 0 < float(rows[1][1]) <= 60 * n and 0 < float(rows[12][1]) <= 41 * n and float(rows[1][7]) > 0   # discharges at noon
    r = CliRunner().invoke(main, ["battery", str(f), *args, "--fleet", str(g), "--bin", "0"])
    assert r.exit_code != 0
