"""The fleet series on the GPU (tmh_set_series, BatchedSim.enable_series): integer sums,
so every comparison with the traces' sums (series.from_traces) is bit for bit."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth, a_oracle, a_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _sim(n, start, prec="fp32", chain0=0, mp=None, horizon=None, **kw):
    from tmhpvsim_amd.engine import BatchedSim
    return BatchedSim(n, start, tz=A_TZ, params=mp, precision=prec, chain0=chain0, device="cuda:0",
                      horizon=horizon or 86400, **kw)


def _last(sim):
    return sim.L.tmh_engine_last_expand(sim._eng)


def _np(t):
    return t.cpu().numpy()


def _traces(sim, windows, variants=True):
    """pv, meter (the OUT_TRACE3 instantiation) and covered (an OUT_ANY run of a second sim of the
    same chains), window by window; returns numpy [steps, n] arrays and the expansion variants."""
    from tmhpvsim_amd import _lib
    a, b = sim
    pv, meter, cov = [], [], []
    for w in windows:
        o = a.run(w, trace=("pv", "meter", "residual"), window=w)
        va = _last(a)
        c = b.run(w, trace=("covered",), window=w)
        vb = _last(b)
        if variants:
            assert va & 7 == _lib.OUT_TRACE3 and vb & 7 == _lib.OUT_ANY
        pv.append(_np(o["pv"]))
        meter.append(_np(o["meter"]))
        cov.append(_np(c["covered"]))
    return np.concatenate(pv), np.concatenate(meter), np.concatenate(cov)


@functools.lru_cache(maxsize=None)
def a_gpu(prec):
    """Input A on the GPU, once per precision: the series over the windows A_WINDOWS, the traces of
    the same chains, the expected series from them, the guard-band records per window."""
    from tmhpvsim_amd import _lib, series
    kw = dict(prec=prec, chain0=A_CHAIN0, mp=a_params(), horizon=A_STEPS)
    sim = _sim(A_N, A_START, **kw)
    assert sim.path == "time_parallel"
    raw = sim.enable_series(A_STEPS)
    guards, variants = [], []
    for w in A_WINDOWS:
        sim.run(w, trace=(), window=w)
        variants.append(_last(sim))
        guards.append(sim.guard_records())
    torch.cuda.synchronize()
    pv, meter, cov = _traces((_sim(A_N, A_START, **kw), _sim(A_N, A_START, **kw)), A_WINDOWS)
    want = series.from_traces(pv, meter, cov)
    return dict(raw=_np(raw), want=want, pv=pv, meter=meter, cov=cov, status=sim.status(), guards=guards,
                variants=variants, fp64=_lib.OUT_FP64 if prec == "fp64" else 0)


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_series_equals_the_traces_sums(prec):
    """The main test: all four columns bit for bit, over two windows (the second off the
    four-step grid), chains faulted at construction and inside the window, night and day."""
    from tmhpvsim_amd import _lib
    g = a_gpu(prec)
    a_has_teeth(g["pv"], g["cov"], g["status"])
    assert g["variants"] == [_lib.OUT_SERIES | g["fp64"]] * len(A_WINDOWS)
    if prec == "fp32":   # the windows hold seconds the fixup replaced
        assert max(g["guards"]) > 0, g["guards"]
    else:
        assert g["guards"] == [0] * len(A_WINDOWS)
    for col in range(4):
        np.testing.assert_array_equal(g["raw"][0, :, col], g["want"][0, :, col], err_msg=f"column {col}")
    assert (g["raw"][0, :, 0] == 0).any() and (g["raw"][0, :, 0] > 0).any()
    assert g["raw"][0, :, 2].min() < g["raw"][0, :, 2].max() < A_N


def test_series_pipelined_windows_same_bits():
    """run() over several windows (the pipelined run_windows path) adds the same series."""
    sim = _sim(A_N, A_START, prec="fp32", chain0=A_CHAIN0, mp=a_params(), horizon=A_STEPS)
    raw = sim.enable_series(A_STEPS)
    sim.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(raw), a_gpu("fp32")["want"])


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-5), ("fp64", 1e-12)])
def test_series_against_the_oracle(prec, tol):
    """Counts exact; sums within the quantisation bound n_ok 2^-(K+1) W plus the project's bar
    (1e-12 fp64, 1e-5 fp32) on the row's sum of |v_ref|."""
    from tmhpvsim_amd import series
    ref, g = a_oracle(), a_gpu(prec)
    a_has_teeth(ref["pv"], ref["covered"], ref["status"])
    np.testing.assert_array_equal(g["status"], ref["status"])
    ok = ref["covered"] != 255
    n_ok = ok.sum(axis=1)
    np.testing.assert_array_equal(g["raw"][0, :, 2], n_ok)
    np.testing.assert_array_equal(g["raw"][0, :, 3], (ref["covered"] == 1).sum(axis=1))
    for col, key in ((0, "pv"), (1, "meter")):
        v = np.where(ok, ref[key], 0.0)
        err = np.abs(g["raw"][0, :, col] / 2.0 ** series.FRAC_BITS - v.sum(axis=1))
        bound = n_ok * 2.0 ** -(series.FRAC_BITS + 1) + tol * np.abs(v).sum(axis=1)
        worst = int(np.argmax(err - bound))
        print(f"{prec} {key}: worst row {worst}: err {err[worst]:.3e} W, bound {bound[worst]:.3e} W")
        assert (err <= bound).all(), (key, worst, err[worst], bound[worst])


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("n,gc", [(1300, 512), (64, 0)])
def test_series_shapes(n, gc, prec):
    """1,300 chains in groups of 512 (a partial last group of 276, a partial wavefront, three
    workgroups of the 512-wide kernel) and a single wavefront; 700 steps across sunrise."""
    from tmhpvsim_amd import series
    start, steps = "2019-09-05 06:58:00", 701
    kw = dict(prec=prec, chain0=A_CHAIN0, mp=a_params(), horizon=steps)
    sim = _sim(n, start, **kw)
    raw = sim.enable_series(steps, group_chains=gc)
    assert tuple(raw.shape) == (3 if gc else 1, steps, 4)
    sim.run(steps, trace=())
    out = _sim(n, start, **kw).run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    pv, cov = _np(out["pv"]), _np(out["covered"])
    assert (np.nan_to_num(pv).max(axis=1) == 0).any() and (np.nan_to_num(pv) > 0).any()   # night and daylight
    if n > 1000:
        assert (cov[0] == 255).any()                                                       # construction faults
    want = series.from_traces(pv, _np(out["meter"]), cov, group_chains=gc)
    np.testing.assert_array_equal(_np(raw), want)
    if gc:
        assert want[2, :, 2].max() <= 276 and want[2, :, 2].max() > 200


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_statistics_unperturbed_by_the_series(prec):
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = dict(prec=prec, chain0=A_CHAIN0, mp=a_params(), horizon=steps)
    both, stats, ser = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats()
    stats.enable_stats()
    ra, rc = both.enable_series(steps), ser.enable_series(steps)
    for s in (both, stats, ser):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and int(ra[..., 2].sum()) > 0
    # the histogram counts the series' ok chain-seconds
    assert int(both.hist.sum()) == int(ra[..., 2].sum())


def test_series_per_chain_sites():
    from oracle import oracle as O
    from tmhpvsim_amd import _lib, series
    from tmhpvsim_amd.params import ModelParams, site_grid
    n, steps, start = 512, 9001, "2019-06-21 02:30:00"
    sites = site_grid(32, 16)
    mp = ModelParams(seed=0x51E)
    sim = _sim(n, start, mp=mp, horizon=steps, sites=sites)
    raw = sim.enable_series(steps)
    sim.run(steps, trace=())
    assert _last(sim) == _lib.OUT_SERIES | _lib.OUT_SITES
    tr = _sim(n, start, mp=mp, horizon=steps, sites=sites)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    assert _last(tr) == _lib.OUT_ANY | _lib.OUT_SITES
    torch.cuda.synchronize()
    want = series.from_traces(out["pv"], out["meter"], out["covered"])
    np.testing.assert_array_equal(_np(raw), want)
    ref = O.run(mp, 0, n, steps, start, tz=A_TZ, n_threads=8, sites=sites, outputs=("pv",))
    pv = ref["pv"][:, ref["status"] == 0]
    first = np.argmax(pv > 0, axis=0)
    assert first.max() - first.min() > 60 * 60      # sunrise spreads over the grid's longitudes / latitudes


def test_two_sims_share_one_buffer():
    from tmhpvsim_amd import series
    n, steps, start = 300, 2000, "2019-09-05 06:30:00"

    def fleet():
        buf = torch.zeros(1, steps, 4, dtype=torch.int64, device="cuda:0")
        for c0 in (5000, 9000):
            s = _sim(n, start, chain0=c0, mp=a_params(), horizon=steps)
            assert s.enable_series(steps, buffer=buf) is buf
            s.run(steps, trace=())
        torch.cuda.synchronize()
        return _np(buf)

    got = fleet()
    want = 0
    for c0 in (5000, 9000):
        out = _sim(n, start, chain0=c0, mp=a_params(), horizon=steps).run(steps, trace=("covered", "pv", "meter"))
        want = want + series.from_traces(out["pv"], out["meter"], out["covered"])
    np.testing.assert_array_equal(got, want)
    assert got[0, :, 2].max() > n                     # both sims' chains in one row
    np.testing.assert_array_equal(fleet(), got)      # a second run: the same bits


def test_every_refusal():
    """Each case of the validation list is refused with TMH_E_INVAL before anything is launched:
    the chains' state and the series stay as they were.  Through the C-ABI (tmh_run, tmh_step's
    halves), then BatchedSim's own refusals."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"

    def refused(sim, match, step0=0, k=100, trace=None, inj=None):
        before = sim.state.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k,
                       C.byref(inj) if inj is not None else None, C.byref(tr), None, C.c_void_p(ws.data_ptr()),
                       ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike (a plan is chain-independent)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k,
                            C.byref(inj) if inj is not None else None, C.byref(tr), None, plan, scr,
                            ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state)
        assert not bool(sim.series_raw.any())

    sim = _sim(n, start, horizon=1000)
    sim.enable_series(500)
    out = torch.zeros(100, n, dtype=torch.float32, device="cuda:0")
    cov = torch.zeros(100, n, dtype=torch.uint8, device="cuda:0")
    refused(sim, "traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))   # a trace beside the series
    refused(sim, "traces", trace=_lib.Trace(None, cov.data_ptr(), None, None, None, n))
    assert not bool(out.any()) and not bool(cov.any())
    refused(sim, "outside the series", step0=0, k=501)                     # past the series' end
    refused(sim, "outside the series", step0=450, k=100)
    sim.enable_series(500, step0=10)
    refused(sim, "outside the series", step0=0, k=100)                     # before its start
    sim.enable_series(500)
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    _lib.check(L.tmh_set_chain_ids(sim._eng, C.c_void_p(ids.data_ptr()), n))
    refused(sim, "compacted")                                              # compaction active
    _lib.check(L.tmh_set_chain_ids(sim._eng, None, 0))
    buf = torch.zeros(1, 500, 4, dtype=torch.int64, device="cuda:0")
    one = _lib.Series(buf.data_ptr(), 0, 500, 512, 1, 0)                   # 1 group x 512 chains < 600
    _lib.check(L.tmh_set_series(sim._eng, C.byref(one)))
    sim.series_raw = buf
    refused(sim, "n_chains")
    for gc, ng in ((100, 6), (256, 3), (0, 2)):                            # a bad group_chains: the setter refuses
        bad = _lib.Series(buf.data_ptr(), 0, 500, gc, ng, 0)
        assert L.tmh_set_series(sim._eng, C.byref(bad)) == -1 and b"group_chains" in L.tmh_last_error()

    seq = _sim(64, start, horizon=1000, kernel_path="sequential")          # the sequential path
    seq.enable_series(500)
    refused(seq, "time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), device="cuda:0", injected=inj,
                      horizon=1000)
    isim.enable_series(500)
    refused(isim, "time-parallel", inj=isim._us)
    mp = ModelParams()
    mp.inverter = dict(mp.inverter, Paco=float(L.tmh_series_max_w()))       # Paco >= TMH_SERIES_MAX_W
    big = _sim(64, start, mp=mp, horizon=1000)
    big.enable_series(500)
    refused(big, "Paco")

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_series(500)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="compacted"):
        sim.run(200, trace=(), window=100, compact=True)
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the series"):
        sim.run(600, trace=(), window=200)
    with pytest.raises(ValueError):
        sim.enable_series(500, group_chains=100)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.series_raw.any())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    assert int(sim.series_raw[0, :100, 2].min()) > 0 and not bool(sim.series_raw[0, 100:].any())


def test_fleet_cli(tmp_path):
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import main
    from tmhpvsim_amd.params import ModelParams
    f = tmp_path / "fleet.csv"
    r = CliRunner().invoke(main, ["fleet", str(f), "--batch", "300", "--seconds", "1500", "--bin", "60", "--no-realtime"])
    assert r.exit_code == 0, r.output
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["time", "n_ok", "meter", "pv", "residual load", "covered"] and len(rows) == 1 + 25
    mp = ModelParams(seed=0x5EED)
    sim = _sim(300, "2019-09-06T12:00:00", mp=mp, horizon=1500)
    sim.enable_series(1500)
    sim.run(1500, trace=())
    want = sim.series(bin_s=60, mean=True)
    assert rows[1][0] == "2019-09-06 12:00:00" and rows[2][0] == "2019-09-06 12:01:00"
    for i, row in enumerate(rows[1:]):
        assert int(row[1]) == int(want["n_ok"][0, i]) > 0
        got = [float(x) for x in row[2:]]
        assert got == [float(want[k][0, i]) for k in ("meter", "pv", "residual", "covered")]
    assert float(rows[1][3]) > 0                     # noon: the fleet produces
