"""Interval metering on the GPU (tmh_set_intervals, BatchedSim.enable_intervals): integer
sums, so every comparison with the traces' sums (intervals.from_traces) is bit for bit.
The expected table always comes from traces of separate sims of the same chains (pv /
meter / residual through OUT_TRACE3, covered through OUT_ANY), never from the code under
test."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth, a_oracle, a_params
from test_gpu_series import _last, _np, _sim, _traces, a_gpu

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IV = 900


def _kw(prec, steps=A_STEPS):
    return dict(prec=prec, chain0=A_CHAIN0, mp=a_params(), horizon=steps)


@functools.lru_cache(maxsize=None)
def a_iv(prec):
    """Input A with interval metering, once per precision: the table over the windows A_WINDOWS
    (900-s intervals), the expected table from the traces of the same chains (test_gpu_series.a_gpu:
    separate sims), the guard-band records per window."""
    from tmhpvsim_amd import intervals
    sim = _sim(A_N, A_START, **_kw(prec))
    assert sim.path == "time_parallel"
    raw = sim.enable_intervals(A_STEPS, IV)
    assert tuple(raw.shape) == (13, 4, A_N)
    guards, variants = [], []
    for w in A_WINDOWS:
        sim.run(w, trace=(), window=w)
        variants.append(_last(sim))
        guards.append(sim.guard_records())
    torch.cuda.synchronize()
    g = a_gpu(prec)
    want = intervals.from_traces(g["pv"], g["meter"], g["cov"], IV)
    return dict(raw=_np(raw), want=want, guards=guards, variants=variants, status=sim.status())


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_intervals_equal_the_traces_sums(prec):
    """The main test: all four columns bit for bit, over two windows (the second off the
    four-step grid), chains faulted at construction and inside the window, night and day."""
    from tmhpvsim_amd import _lib
    g, t = a_iv(prec), a_gpu(prec)
    a_has_teeth(t["pv"], t["cov"], t["status"])
    assert g["variants"] == [_lib.OUT_INTERVALS | t["fp64"]] * len(A_WINDOWS)
    assert all(v & 7 == _lib.OUT_INTERVALS for v in g["variants"])
    if prec == "fp32":   # the windows hold seconds the fixup replaced
        assert max(g["guards"]) > 0, g["guards"]
    else:
        assert g["guards"] == [0] * len(A_WINDOWS)
    for col in range(4):
        np.testing.assert_array_equal(g["raw"][:, col], g["want"][:, col], err_msg=f"column {col}")
    assert (g["raw"][:, 0] == 0).any() and (g["raw"][:, 0] > 0).any()
    assert g["raw"][12, 2].max() == 3 and g["raw"][:12, 2].max() == IV          # the last partial interval
    n_ok = g["raw"][:, 2].sum(axis=0)
    assert (n_ok == 0).sum() >= 10 and ((n_ok > 0) & (n_ok < A_STEPS)).sum() >= 3


B_START, B_STEPS, B_WINDOWS, B_LEAD = "2019-09-05 06:58:00", 701, (300, 401), 3


@functools.lru_cache(maxsize=None)
def b_traces(n, prec):
    """The boundary tests' traces: n chains, 701 steps from 06:58 across sunrise, as windows 300 + 401."""
    kw = _kw(prec, B_STEPS)
    pv, meter, cov = _traces((_sim(n, B_START, **kw), _sim(n, B_START, **kw)), B_WINDOWS)
    for a in (pv, meter, cov):
        a.setflags(write=False)
    return pv, meter, cov


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("interval_s", [7, 60, 128, 900])
@pytest.mark.parametrize("n", [1300, 64])
def test_interval_boundaries(n, interval_s, prec):
    """Boundaries inside four-second groups (7), several in a 128-s block (60), one per block
    (128), a single partial interval (900); the origin three steps before the run, so no
    interval edge coincides with a window edge; a partial wavefront and construction faults."""
    from tmhpvsim_amd import _lib, intervals
    pv, meter, cov = b_traces(n, prec)
    assert (np.nan_to_num(pv).max(axis=1) == 0).any() and (np.nan_to_num(pv) > 0).any()   # night and daylight
    if n > 1000:
        assert (cov[0] == 255).any()                                                       # construction faults
    sim = _sim(n, B_START, **_kw(prec, B_STEPS))
    raw = sim.enable_intervals(B_STEPS + B_LEAD, interval_s, step0=-B_LEAD)
    for w in B_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) & 7 == _lib.OUT_INTERVALS
    torch.cuda.synchronize()
    want = intervals.from_traces(pv, meter, cov, interval_s, origin=B_LEAD)
    assert tuple(raw.shape) == want.shape == (-(-(B_STEPS + B_LEAD) // interval_s), 4, n)
    for w0 in np.cumsum((0,) + B_WINDOWS):
        assert interval_s > B_STEPS or (int(w0) + B_LEAD) % interval_s != 0
    np.testing.assert_array_equal(_np(raw), want)


def test_intervals_pipelined_windows_same_bits():
    """run() over several windows (the pipelined run_windows path) adds the same table."""
    sim = _sim(A_N, A_START, **_kw("fp32"))
    raw = sim.enable_intervals(A_STEPS, IV)
    sim.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(raw), a_iv("fp32")["want"])
    np.testing.assert_array_equal(_np(raw), a_iv("fp32")["raw"])


def test_intervals_compacted_windows_same_bits():
    """compact=True: from the second window on only the live chains run, in dense slots; a
    slot's column is its chain's (ids[slot]), so the table is the uncompacted one."""
    g, t = a_iv("fp32"), a_gpu("fp32")
    a_has_teeth(t["pv"], t["cov"], t["status"])
    sim = _sim(A_N, A_START, **_kw("fp32"))
    raw = sim.enable_intervals(A_STEPS, IV)
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
def test_statistics_unperturbed_by_the_intervals(prec, spec):
    """Statistics beside the intervals are the statistics-only run's, bit for bit, and the table is
    the intervals-only one.  `offset` and `huge` are histogram specs the fp32 kernels must bin in
    fp64 (StatsView::bin64: the OUT_INTERVALS | OUT_B64 instantiations); the test asserts of its
    input that fp32 binning would put some of the run's seconds into another bin, so launching the
    plain fp32 kernel for them would show."""
    from test_gpu_trace3 import HISTS
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw(prec, steps)
    both, stats, ivl = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats(**HISTS[spec])
    stats.enable_stats(**HISTS[spec])
    ra, rc = both.enable_intervals(steps, 600), ivl.enable_intervals(steps, 600)
    for s in (both, stats, ivl):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and int(ra[:, 2].sum()) > 0
    # the histogram counts the intervals' ok chain-seconds (out-of-range seconds go to the edge bins)
    assert int(both.hist.sum()) == int(ra[:, 2].sum())
    if prec == "fp32" and spec != "default":
        h = HISTS[spec]
        res = _np(_sim(n, start, **kw).run(steps, trace=("residual",))["residual"])
        res = res[~np.isnan(res)].astype(np.float64)
        nb, scale = h["n_bins"], h["n_bins"] / (h["hi"] - h["lo"])
        b64 = np.clip(np.floor((res - h["lo"]) * scale), 0, nb - 1).astype(np.int64)
        x32 = (res * np.float64(np.float32(scale)) + np.float64(np.float32(-h["lo"] * scale))).astype(np.float32)
        b32 = np.clip(x32, 0, nb - 1).astype(np.int64)
        np.testing.assert_array_equal(np.bincount(b64, minlength=nb), _np(stats.hist))   # the kernels bin in fp64
        assert int((b32 != b64).sum()) > 0


def test_two_batches_fill_one_table():
    """Chains [5000, 5512) and [5512, 6000) as two sims writing column slices of one buffer."""
    big = torch.zeros(13, 4, A_N, dtype=torch.int64, device="cuda:0")
    for a, b in ((0, 512), (512, A_N)):
        s = _sim(b - a, A_START, prec="fp32", chain0=A_CHAIN0 + a, mp=a_params(), horizon=A_STEPS)
        view = big[:, :, a:b]
        got = s.enable_intervals(A_STEPS, IV, buffer=view)
        assert got is view and s._intervals.ld == A_N
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), a_iv("fp32")["raw"])
    with pytest.raises(ValueError, match="strides"):
        s.enable_intervals(A_STEPS, IV, buffer=big[:, :, :2 * s.n:2])     # chains not contiguous
    s.enable_intervals(None)


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_intervals_sum_to_the_fleet_series(prec):
    """Two independent kernels: the interval table summed over the chains equals the GPU fleet
    series of the same run configuration summed over each interval's seconds, all four columns."""
    ser = a_gpu(prec)["raw"][0]                                    # [steps, 4]
    want = np.add.reduceat(ser, np.arange(0, A_STEPS, IV), axis=0)
    np.testing.assert_array_equal(a_iv(prec)["raw"].sum(axis=2), want)


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-5), ("fp64", 1e-12)])
def test_intervals_against_the_oracle(prec, tol):
    """Counts exact; sums per cell within the quantisation bound n_ok 2^-(K+1) W plus the
    project's bar (1e-12 fp64, 1e-5 fp32) on the cell's sum of |v_ref|."""
    from tmhpvsim_amd import intervals
    ref, g = a_oracle(), a_iv(prec)
    a_has_teeth(ref["pv"], ref["covered"], ref["status"])
    np.testing.assert_array_equal(g["status"], ref["status"])
    ok = ref["covered"] != 255
    edges = np.arange(0, A_STEPS, IV)
    n_ok = np.add.reduceat(ok.astype(np.int64), edges, axis=0)
    np.testing.assert_array_equal(g["raw"][:, 2], n_ok)
    np.testing.assert_array_equal(g["raw"][:, 3], np.add.reduceat((ref["covered"] == 1).astype(np.int64), edges, axis=0))
    for col, key in ((0, "pv"), (1, "meter")):
        v = np.where(ok, ref[key], 0.0)
        err = np.abs(g["raw"][:, col] / 2.0 ** intervals.FRAC_BITS - np.add.reduceat(v, edges, axis=0))
        bound = n_ok * 2.0 ** -(intervals.FRAC_BITS + 1) + tol * np.add.reduceat(np.abs(v), edges, axis=0)
        worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        print(f"{prec} {key}: worst cell {worst}: err {err[worst]:.3e} W s, bound {bound[worst]:.3e} W s")
        assert (err <= bound).all(), (key, worst, err[worst], bound[worst])


@pytest.mark.parametrize("spec", ["default", "huge"])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_intervals_per_chain_sites(prec, spec):
    """The per-chain-sites kernels, with statistics beside the intervals: `huge` is a histogram
    spec that the fp32 kernel bins in fp64 (its OUT_B64 instantiation)."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib, intervals
    from tmhpvsim_amd.params import ModelParams, site_grid
    n, steps, start = 512, 3000, "2019-06-21 04:45:00"
    sites = site_grid(32, 16)
    mp = ModelParams(seed=0x51E)
    sim = _sim(n, start, prec=prec, mp=mp, horizon=steps, sites=sites)
    raw = sim.enable_intervals(steps + 1, 450, step0=-1)
    stats = _sim(n, start, prec=prec, mp=mp, horizon=steps, sites=sites)
    for s in (sim, stats):
        s.enable_stats(**HISTS[spec])
    stats.run(steps, trace=(), window=1700)
    assert _last(stats) & 7 == _lib.OUT_STATS
    sim.run(steps, trace=(), window=1700)
    assert _last(sim) == _lib.OUT_INTERVALS | _lib.OUT_SITES | (_lib.OUT_FP64 if prec == "fp64" else 0)
    tr = _sim(n, start, prec=prec, mp=mp, horizon=steps, sites=sites)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    pv = _np(out["pv"])
    lit = (pv > 0).any(axis=0)
    first = np.argmax(pv[:, lit] > 0, axis=0)                      # sunrise spreads over the grid's sites
    # daylight from the first step on some sites, a whole 128-s block of night first on others
    assert first.min() == 0 and first.max() > 128, (int(lit.sum()), first.min(), first.max())
    np.testing.assert_array_equal(_np(raw), intervals.from_traces(out["pv"], out["meter"], out["covered"], 450, origin=1))
    assert int(stats.hist.sum()) == int(raw[:, 2].sum()) > 0
    assert torch.equal(sim.hist, stats.hist)
    assert torch.equal(sim.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message before anything is launched: the
    chains' state stays as it was and the table all zeros."""
    from tmhpvsim_amd import _lib
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"

    def refused(sim, match, step0=0, k=100, trace=None):
        before = sim.state.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, None, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, None, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if sim.path == "time_parallel" and trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state)
        assert not bool(sim.intervals_raw.any())

    sim = _sim(n, start, horizon=1000)
    sim.enable_intervals(500, 60)
    out = torch.zeros(100, n, dtype=torch.float32, device="cuda:0")
    refused(sim, "traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))   # a trace beside the intervals
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # a fleet series beside them
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    refused(sim, "outside the intervals", step0=0, k=501)                  # past the end
    refused(sim, "outside the intervals", step0=450, k=100)
    sim.enable_intervals(500, 60, step0=10)
    refused(sim, "outside the intervals", step0=0, k=100)                  # before the origin
    buf = sim.enable_intervals(500, 60)
    small = _lib.Intervals(buf.data_ptr(), 0, 500, 60, n - 1)             # ld too small
    _lib.check(L.tmh_set_intervals(sim._eng, C.byref(small)))
    refused(sim, "ld")
    for bad in (_lib.Intervals(buf.data_ptr() + 4, 0, 500, 60, n), _lib.Intervals(None, 0, 500, 60, n),
                _lib.Intervals(buf.data_ptr(), 0, 500, 0, n)):             # the setter refuses a bad struct
        assert L.tmh_set_intervals(sim._eng, C.byref(bad)) == -1 and L.tmh_last_error()
    seq = _sim(64, start, horizon=1000, kernel_path="sequential")          # the sequential path
    seq.enable_intervals(500, 60)
    refused(seq, "time-parallel")

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_intervals(500, 60)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the intervals"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.intervals_raw.any())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    assert int(sim.intervals_raw[0, 2].min()) >= 0 and int(sim.intervals_raw[:2, 2].sum()) > 0
    assert not bool(sim.intervals_raw[2:].any())
    assert L.tmh_set_intervals(sim._eng, None) == 0                        # NULL: off


def test_intervals_cli(tmp_path):
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import main
    from tmhpvsim_amd.params import ModelParams
    f, z = tmp_path / "iv.csv", tmp_path / "iv.npz"
    r = CliRunner().invoke(main, ["intervals", str(f), "--batch", "300", "--seconds", "1500", "--interval", "600",
                                  "--no-realtime", "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["time", "meter", "pv", "residual load"] and len(rows) == 1 + 3
    sim = _sim(300, "2019-09-06T12:00:00", mp=ModelParams(seed=0x5EED), horizon=1500)
    sim.enable_intervals(1500, 600)
    sim.run(1500, trace=())
    want = sim.intervals()
    assert [row[0] for row in rows[1:]] == ["2019-09-06 12:00:00", "2019-09-06 12:10:00", "2019-09-06 12:20:00"]
    for k, row in enumerate(rows[1:]):
        assert [float(x) for x in row[1:]] == [float(want[key][k, 0]) for key in ("meter", "pv", "residual")]
    assert float(rows[1][2]) > 0                     # noon: chain 0 produces
    saved = np.load(z)
    np.testing.assert_array_equal(saved["raw"], _np(sim.intervals_raw))
    assert saved["energy_wh_pv"].shape == (3, 300) and int(saved["interval_s"]) == 600
    assert saved["n_ok"][2].max() == 300             # the last partial interval: 300 s
