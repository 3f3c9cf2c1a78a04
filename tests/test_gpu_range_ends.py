"""The integer table kinds on the GPU at the ends of the ranges tmhpvsim.h documents (range_util): a fleet clipped
at an inverter one quantum under TMH_SERIES_MAX_W, whose half-wave partials reach 2^31 - 32,768; batteries and dispatch
rules with every parameter at an end of its range, 40-bit states of charge and 17-bit kd; out-of-range values written
over the device tensors after enable_*, which only the kernels' clamps stand against; and the sweeps at their sixteen
variants.  Everything is an integer, so every comparison is bit for bit, and every expected table comes from traces of
separate sims of the same chains through the plain loops (the from_traces functions), never from the kernels under
test.  test_range_ends_cpu asserts on the oracle's traces that these inputs reach the ends they are meant to reach."""
import functools

import numpy as np
import pytest

import range_util as R
from battery_util import uniform
from dispatch_sweep_util import rolled
from dispatch_util import identities, soc_changes
from range_util import (C_LEAD, C_START, C_STEPS, C_WINDOWS, CAP_TOP, D_CHAIN0, D_N, D_START, D_STEPS, D_WINDOWS,
                        assert_corners_bite, assert_d_bites, clip, corner_counts, corners, d_params, poison, poison_soc,
                        rolled_corners)
from series_util import A_N, A_START, A_STEPS, A_WINDOWS, a_has_teeth
from sweep_util import variants
from test_gpu_battery import _identities, _soc_changes
from test_gpu_battery_fleet import _row_identities
from test_gpu_demand import _keys_sane
from test_gpu_registers import _identity, _kw, _run_windows
from test_gpu_series import _last, _np, _sim, _traces
from test_gpu_storage import IV, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARAMS, SOC0 = corners()
GC = 512
CLAMP_N, CLAMP_IV = 320, 60
SWEEP_N, SWEEP_IV = 1300, 60


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")          # (a copy: the cached inputs are read-only)


def _kwd(prec):
    return _kw(prec, D_STEPS, mp=d_params())


def test_the_inputs_are_the_boundary_tests():
    import test_gpu_registers as G
    assert (R.C_START, R.C_STEPS, R.C_WINDOWS, R.C_LEAD) == (G.C_START, G.C_STEPS, G.C_WINDOWS, G.C_LEAD)
    assert D_CHAIN0 == 5000 and D_N % 32 == 8 and D_N == A_N


# ------------------------------------------------------------------ 1. input D
@functools.lru_cache(maxsize=None)
def d_traces(prec):
    """Input D's traces of separate sims, once per precision: (pv, meter, covered [steps, n], status [n])."""
    a, b = _sim(D_N, D_START, **_kwd(prec)), _sim(D_N, D_START, **_kwd(prec))
    assert a.path == "time_parallel"
    pv, meter, cov = _traces((a, b), D_WINDOWS)
    status = a.status()
    for arr in (pv, meter, cov, status):
        arr.setflags(write=False)
    c = assert_d_bites(pv, cov, status)
    print(f"D {prec}: {c}")
    np.testing.assert_array_equal(status == 1, cov[0] == 255)
    return pv, meter, cov, status


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("gc", [0, GC])
def test_series_at_the_int32_bound(gc, prec):
    """The fleet series of D, one group and groups of 512: half-waves of 32 lanes at q(Paco) sum to 2^31 - 32,768 in
    thousands of seconds (range_util.assert_d_bites, on these traces).  The fp32 expectation is the fp32 traces', that
    is, after the fixup; the guard-band records are printed, not asserted."""
    from tmhpvsim_amd import _lib, series
    pv, meter, cov, status = d_traces(prec)
    sim = _sim(D_N, D_START, **_kwd(prec))
    raw = sim.enable_series(D_STEPS, group_chains=gc)
    variants_, guards = _run_windows(sim, D_WINDOWS)
    print(f"D {prec} group_chains {gc}: guard-band records per window {guards}")
    assert variants_ == [_lib.OUT_SERIES | (_lib.OUT_FP64 if prec == "fp64" else 0)] * len(D_WINDOWS)
    want = series.from_traces(pv, meter, cov, group_chains=gc)
    got = _np(raw)
    assert got.shape == want.shape == (2 if gc else 1, D_STEPS, 4)
    for col in range(4):
        np.testing.assert_array_equal(got[..., col], want[..., col], err_msg=f"column {col}")
    np.testing.assert_array_equal(sim.status(), status)
    assert int(want[..., 0].max()) > 400 * R.D_Q                           # hundreds of chains at Paco in one row


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("interval_s", [900, 7])
@pytest.mark.parametrize("kind", ["registers", "demand"])
def test_registers_and_demand_at_paco(kind, interval_s, prec):
    """The import / export registers and the demand registers of D: a second's export is q(Paco) - q(meter), up to
    2^26 - 2^10, and the peak-export key carries it."""
    from tmhpvsim_amd import _lib, demand, registers, series
    pv, meter, cov, status = d_traces(prec)
    mod = demand if kind == "demand" else registers
    sim = _sim(D_N, D_START, **_kwd(prec))
    raw = getattr(sim, "enable_" + kind)(D_STEPS, interval_s)
    variants_, guards = _run_windows(sim, D_WINDOWS)
    print(f"D {prec} {kind} {interval_s}: guard-band records per window {guards}")
    out = _lib.OUT_DEMAND if kind == "demand" else _lib.OUT_REGISTERS
    assert [v & 7 for v in variants_] == [out] * len(D_WINDOWS)
    want = mod.from_traces(pv, meter, cov, interval_s)
    got = _np(raw)
    assert got.shape == want.shape
    for col in range(want.shape[1]):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg=f"column {col}")
    _identity(got)
    assert not got[:, :, status == 1].any()
    ok = ~(np.isnan(pv) | np.isnan(meter) | (cov == 255))
    d = np.where(ok, series.quantize(pv) - series.quantize(meter), 0)
    assert int(d.max()) > R.D_Q - (9000 << 12)                             # (of the traces: the export side is near q(Paco))
    if kind == "demand":
        _keys_sane(got, interval_s)
        assert int(demand.unpack(got[:, 7])[0].max()) == int(d.max())


def _d_fleet(par, soc0):
    """D with the battery kind and its fleet series in groups of 512; everything checked against the traces' loops.
    Returns the fleet rows and the traces' ok mask."""
    from tmhpvsim_amd import _lib, battery
    pv, meter, cov, status = d_traces("fp64")
    sim = _sim(D_N, D_START, **_kwd("fp64"))
    raw = sim.enable_battery(D_STEPS, IV, params=_dev(par), soc=_dev(soc0))
    fl = sim.enable_battery_fleet(D_STEPS, group_chains=GC)
    variants_, guards = _run_windows(sim, D_WINDOWS)
    assert variants_ == [_lib.OUT_BATTERY_FLEET | _lib.OUT_FP64] * len(D_WINDOWS) and guards == [0] * len(D_WINDOWS)
    want, end = battery.fleet_from_traces(pv, meter, cov, params=par, soc0=soc0, group_chains=GC)
    got = _np(fl)
    assert got.shape == want.shape == (2, D_STEPS, 8)
    for col in range(8):
        np.testing.assert_array_equal(got[..., col], want[..., col], err_msg=f"column {col}")
    table, tend = battery.from_traces(pv, meter, cov, IV, params=par, soc0=soc0)
    np.testing.assert_array_equal(_np(raw), table)
    np.testing.assert_array_equal(_np(sim.soc), end)
    np.testing.assert_array_equal(tend, end)
    _identities(_np(raw))
    _soc_changes(_np(raw), soc0, _np(sim.soc))
    _row_identities(got, [par[0, :GC].sum(), par[0, GC:].sum()])
    dead = status == 1
    assert dead.any() and not _np(raw)[:, :, dead].any() and (_np(sim.soc)[dead] == soc0[dead]).all()
    return got, ~(np.isnan(pv) | np.isnan(meter) | (cov == 255))


def test_fleet_of_full_batteries():
    """Every battery holds 2^40 - 1 and neither charges nor discharges: every ok lane carries 0xFFFFF in both 20-bit
    halves of its state of charge at every second, so column 6 is n_ok x (2^40 - 1) row by row."""
    par = uniform(D_N, CAP_TOP, 0, 0)
    soc0 = np.full(D_N, CAP_TOP, dtype=np.int64)
    got, ok = _d_fleet(par, soc0)
    n_ok = np.stack([ok[:, :GC].sum(axis=1), ok[:, GC:].sum(axis=1)])
    np.testing.assert_array_equal(got[..., 2], n_ok)
    np.testing.assert_array_equal(got[..., 6], n_ok * CAP_TOP)
    assert int(n_ok.max()) > 400 and not got[..., 7].any()


def test_fleet_of_corner_batteries():
    """The corner recipe's batteries behind D's clipped fleet: exports of q(Paco) - q(meter) per lane beside states of
    charge at both ends of 40 bits."""
    got, _ = _d_fleet(PARAMS[:6], SOC0)
    assert int(got[..., 6].max()) > 100 * (CAP_TOP // 2) and int(got[..., 7].max()) > 0


# ------------------------------------------------------------------ 2. the corner recipe on input A
@functools.lru_cache(maxsize=None)
def a_corner_want():
    """The expected dispatch table and end state of input A (60 modules) at the corner recipe, from the storage tests'
    traces; the table's counts must clear the floors test_range_ends_cpu asserts on the oracle's traces."""
    from tmhpvsim_amd import dispatch
    t = a60_gpu()
    want, end = dispatch.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS, soc0=SOC0)
    counts = corner_counts(want, None, PARAMS)
    print(counts)
    assert_corners_bite(counts)
    return want, end


@functools.lru_cache(maxsize=None)
def a_corner_battery_want():
    from tmhpvsim_amd import battery
    t = a60_gpu()
    return battery.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS[:6], soc0=SOC0)


def _dead_untouched(raw, soc, status):
    dead = status == 1
    assert dead.any() and not raw[:, :, dead].any() and (soc[dead] == SOC0[dead]).all()


def test_corner_batteries():
    """enable_battery at the corner recipe's six rows: all ten columns and the state of charge."""
    from tmhpvsim_amd import _lib
    t = a60_gpu()
    want, end = a_corner_battery_want()
    sim = _sim(A_N, A_START, **_kw60())
    raw = sim.enable_battery(A_STEPS, IV, params=_dev(PARAMS[:6]), soc=_dev(SOC0))
    variants_, guards = _run_windows(sim, A_WINDOWS)
    assert variants_ == [_lib.OUT_BATTERY | _lib.OUT_FP64] * len(A_WINDOWS) and guards == [0] * len(A_WINDOWS)
    got, soc = _np(raw), _np(sim.soc)
    a_has_teeth(t["pv"], t["cov"], sim.status())
    for col in range(10):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(soc, end)
    _identities(got)
    _soc_changes(got, SOC0, soc)
    _dead_untouched(got, soc, sim.status())
    assert int((got[:, 8] & CAP_TOP).max()) == CAP_TOP


def test_corner_batteries_with_their_fleet_series():
    """enable_battery_fleet beside the battery kind at the corner recipe: the eight columns of both groups, the table
    and the state of charge as without it."""
    from tmhpvsim_amd import _lib, battery
    t = a60_gpu()
    table, tend = a_corner_battery_want()
    want, end = battery.fleet_from_traces(t["pv"], t["meter"], t["cov"], params=PARAMS[:6], soc0=SOC0, group_chains=GC)
    sim = _sim(A_N, A_START, **_kw60())
    raw = sim.enable_battery(A_STEPS, IV, params=_dev(PARAMS[:6]), soc=_dev(SOC0))
    fl = sim.enable_battery_fleet(A_STEPS, group_chains=GC)
    variants_, guards = _run_windows(sim, A_WINDOWS)
    assert variants_ == [_lib.OUT_BATTERY_FLEET | _lib.OUT_FP64] * len(A_WINDOWS) and guards == [0] * len(A_WINDOWS)
    got, soc = _np(fl), _np(sim.soc)
    for col in range(8):
        np.testing.assert_array_equal(got[..., col], want[..., col], err_msg=f"column {col}")
    np.testing.assert_array_equal(_np(raw), table)
    np.testing.assert_array_equal(soc, end)
    np.testing.assert_array_equal(tend, end)
    _identities(_np(raw))
    _soc_changes(_np(raw), SOC0, soc)
    _row_identities(got, [PARAMS[0, :GC].sum(), PARAMS[0, GC:].sum()])
    _dead_untouched(_np(raw), soc, sim.status())
    assert int(got[..., 6].max()) > 100 * (CAP_TOP // 2)                   # the high halves carry most of the sum


def test_corner_dispatch_windows_and_compaction():
    """enable_dispatch at the corner recipe: all thirteen columns and the state of charge over A_WINDOWS, then one
    compacted run (windows of 3,601 steps, the live chains in dense slots) with the same bits."""
    from tmhpvsim_amd import _lib
    t = a60_gpu()
    want, end = a_corner_want()
    sim = _sim(A_N, A_START, **_kw60())
    raw = sim.enable_dispatch(A_STEPS, IV, params=_dev(PARAMS), soc=_dev(SOC0))
    variants_, guards = _run_windows(sim, A_WINDOWS)
    assert variants_ == [_lib.OUT_DISPATCH | _lib.OUT_FP64] * len(A_WINDOWS) and guards == [0] * len(A_WINDOWS)
    got, soc = _np(raw), _np(sim.soc)
    a_has_teeth(t["pv"], t["cov"], sim.status())
    for col in range(13):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(soc, end)
    identities(got, PARAMS)
    soc_changes(got, SOC0, soc)
    _dead_untouched(got, soc, sim.status())
    comp = _sim(A_N, A_START, **_kw60())
    rawc = comp.enable_dispatch(A_STEPS, IV, params=_dev(PARAMS), soc=_dev(SOC0))
    comp.run(A_STEPS, trace=(), window=3601, compact=True)
    torch.cuda.synchronize()
    assert len(comp.compact_slots) == 3 and min(comp.compact_slots) < A_N, comp.compact_slots
    np.testing.assert_array_equal(_np(rawc), want)
    np.testing.assert_array_equal(_np(comp.soc), end)
    np.testing.assert_array_equal(comp.status(), sim.status())


# ------------------------------------------------------------------ 3. the clamps a lane applies
def _overwrite(tensor, host):
    """The device tensor's contents replaced in place (the kernels read it at every launch)."""
    ptr = tensor.data_ptr()
    tensor.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    torch.cuda.synchronize()
    assert tensor.data_ptr() == ptr
    np.testing.assert_array_equal(_np(tensor), host)


def _c_sim(n):
    return _sim(n, C_START, **_kw60(C_STEPS))


def _run_c(sim):
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
    torch.cuda.synchronize()


@pytest.mark.parametrize("stagger", [False, True], ids=["pattern", "staggered"])
@pytest.mark.parametrize("kind", ["battery", "dispatch"])
def test_lanes_clamp_what_they_load(kind, stagger):
    """Python checks the parameters at enable_* only; a C caller's tensors are never read on the host.  Valid tensors
    are enabled, then overwritten in place: chain i of every row holds hi + 1, -1, INT64_MAX, INT64_MIN or its valid
    value by (i + row) % 5, the state of charge the same against [0, C].  The run equals the loop at the clipped
    parameters and the clipped start; the parameters are read, never written.  staggered: rows 5-8 one chain further
    on (range_util.poison), so that a threshold below 0 meets a power limit above 0 and its lower clamp shows."""
    from tmhpvsim_amd import battery, dispatch
    mod = battery if kind == "battery" else dispatch
    rows, n = len(mod.RANGES), CLAMP_N
    pv, meter, cov = c60_traces(n)
    valid, soc_valid = rolled_corners(1, n)
    valid, soc_valid = valid[0, :rows], soc_valid[0]
    bad = poison(valid, mod.RANGES, stagger=stagger)
    ok = clip(bad, mod.RANGES)
    soc_bad = poison_soc(soc_valid, ok[0], rows)
    want, end = mod.from_traces(pv, meter, cov, CLAMP_IV, origin=C_LEAD, params=ok, soc0=np.clip(soc_bad, 0, ok[0]))
    sim = _c_sim(n)
    raw = getattr(sim, "enable_" + kind)(C_STEPS + C_LEAD, CLAMP_IV, step0=-C_LEAD, params=_dev(valid), soc=_dev(soc_valid))
    par_t = sim.battery_params if kind == "battery" else sim.dispatch_params
    _overwrite(par_t, bad)
    _overwrite(sim.soc, soc_bad)
    _run_c(sim)
    got, soc = _np(raw), _np(sim.soc)
    for col in range(want.shape[1]):
        np.testing.assert_array_equal(got[:, col], want[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(soc, end)
    np.testing.assert_array_equal(_np(par_t), bad)                          # bitwise unchanged
    assert ((soc >= 0) & (soc <= ok[0])).all()
    if kind == "battery":
        _identities(got)
        _soc_changes(got, np.clip(soc_bad, 0, ok[0]), soc)
    else:
        identities(got, ok)
        soc_changes(got, np.clip(soc_bad, 0, ok[0]), soc)


@pytest.mark.parametrize("stagger", [False, True], ids=["pattern", "staggered"])
def test_sweep_lanes_clamp_what_they_load(stagger):
    """The same for the dispatch sweep with five variants (a full group of launches and a group of one): the pattern
    runs on through the rows of the [K, 9, n] tensor and of the [K, n] states of charge."""
    from tmhpvsim_amd import dispatch
    k, n, rows = 5, CLAMP_N, 9
    pv, meter, cov = c60_traces(n)
    valid, soc_valid = rolled_corners(k, n)
    bad = np.stack([poison(valid[v], dispatch.RANGES, shift=v * rows, stagger=stagger) for v in range(k)])
    ok = np.stack([clip(bad[v], dispatch.RANGES) for v in range(k)])
    soc_bad = np.stack([poison_soc(soc_valid[v], ok[v, 0], k * rows + v) for v in range(k)])
    soc_ok = np.clip(soc_bad, 0, ok[:, 0])
    sim = _c_sim(n)
    raw = sim.enable_dispatch_sweep(C_STEPS + C_LEAD, CLAMP_IV, step0=-C_LEAD, params=_dev(valid), soc=_dev(soc_valid))
    _overwrite(sim.dispatch_params, bad)
    _overwrite(sim.soc, soc_bad)
    _run_c(sim)
    got, soc = _np(raw), _np(sim.soc)
    for v in range(k):
        want, end = dispatch.from_traces(pv, meter, cov, CLAMP_IV, origin=C_LEAD, params=ok[v], soc0=soc_ok[v])
        for col in range(13):
            np.testing.assert_array_equal(got[v, :, col], want[:, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(soc[v], end, err_msg=f"variant {v}")
        identities(got[v], ok[v])
        soc_changes(got[v], soc_ok[v], soc[v])
    np.testing.assert_array_equal(_np(sim.dispatch_params), bad)            # bitwise unchanged
    assert ((soc >= 0) & (soc <= ok[:, 0])).all()


# ------------------------------------------------------------------ 4. the sweeps at their maximum
@functools.lru_cache(maxsize=None)
def sweep_want(kind):
    """(params [16, rows, n], soc0 [16, n], tables, end states) of input C under sixteen variants: the sweep's own plain
    loop over the traces (test_range_ends_cpu holds it against from_traces variant by variant)."""
    from tmhpvsim_amd import battery, dispatch
    pv, meter, cov = c60_traces(SWEEP_N)
    if kind == "dispatch":
        par, soc0 = rolled(16, SWEEP_N, "C")
        want, end = dispatch.sweep_from_traces(pv, meter, cov, SWEEP_IV, origin=C_LEAD, params=par, soc0=soc0)
    else:
        par, soc0 = variants(16, SWEEP_N)
        want, end = battery.sweep_from_traces(pv, meter, cov, SWEEP_IV, origin=C_LEAD, params=par, soc0=soc0)
    for a in (par, soc0, want, end):
        a.setflags(write=False)
    return par, soc0, want, end


def _sweep_run(kind, par, soc0):
    from tmhpvsim_amd import _lib
    sim = _c_sim(SWEEP_N)
    raw = getattr(sim, f"enable_{kind}_sweep")(C_STEPS + C_LEAD, SWEEP_IV, step0=-C_LEAD, params=_dev(par), soc=_dev(soc0))
    out = _lib.OUT_DISPATCH_SWEEP if kind == "dispatch" else _lib.OUT_BATTERY_SWEEP
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == out | _lib.OUT_FP64
    torch.cuda.synchronize()
    return _np(raw), _np(sim.soc)


@pytest.mark.parametrize("k", [16, 8])
@pytest.mark.parametrize("kind", ["battery", "dispatch"])
def test_sweeps_at_their_maximum(kind, k):
    """Sixteen variants, the most a sweep takes, and eight: four and two full groups of launches.  Every variant's
    table and state of charge bit for bit against the sweep's loop over the traces, columns 0-3 equal across the
    variants; of the sixteen, the first and the last variant of the fourth group against the kind's own from_traces
    too (all sixteen that way would take longer than any other table test)."""
    from tmhpvsim_amd import battery, dispatch
    assert battery.SWEEP_MAX == dispatch.SWEEP_MAX == 16
    par, soc0, want, end = sweep_want(kind)
    got, soc = _sweep_run(kind, par[:k], soc0[:k])
    assert got.shape == want[:k].shape and soc.shape == (k, SWEEP_N)
    for v in range(k):
        for col in range(want.shape[2]):
            np.testing.assert_array_equal(got[v, :, col], want[v, :, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(soc[v], end[v], err_msg=f"variant {v} soc")
        np.testing.assert_array_equal(got[v, :, :4], got[0, :, :4])
        assert v == 0 or (want[v, :, 4:] != want[v - 1, :, 4:]).any()
    if k == 16:                                                             # the last launch group against the kind's own loop
        pv, meter, cov = c60_traces(SWEEP_N)
        mod = dispatch if kind == "dispatch" else battery
        for v in (12, 15):
            table, tend = mod.from_traces(pv, meter, cov, SWEEP_IV, origin=C_LEAD, params=par[v], soc0=soc0[v])
            np.testing.assert_array_equal(got[v], table, err_msg=f"variant {v}")
            np.testing.assert_array_equal(soc[v], tend, err_msg=f"variant {v} soc")
    if kind == "dispatch" and k == 16:                                      # variants 0-4 as a sweep of their own
        got5, soc5 = _sweep_run(kind, par[:5], soc0[:5])
        np.testing.assert_array_equal(got5, got[:5])
        np.testing.assert_array_equal(soc5, soc[:5])
