"""The PV half on the GPU beyond the default Munich system, against the fp64 oracle.

Every other GPU test runs MODULE_DEFAULT / INVERTER_DEFAULT at 20 C without wind, on Munich or a
European grid facing south.  Here (inputs: tests/pv_util.py; tests/test_pv_inputs_cpu.py shows on the
oracle alone that each set reaches what it is there for):

  1a  a system in which every host-folded constant of the chain shows and the inverter clips;
  1b  128 sites around the world, one per chain: both hemispheres, the date line, polar day and
      night, sunrise and sunset, four tilts and azimuths, sites up to 4,000 m;
  2   the per-second chain itself on real and planted geometry rows (tmh_probe_pv against
      orc_pv_row): every discontinuity and clamp, and the fp32 contract per second -- within
      1e-5 of the oracle or flagged for the fp64 recomputation -- before fixup_kernel repairs it.

Bars: the project's own (tests/test_gpu_parity.py::_check_vs_oracle; fp64 1e-12, fp32 1e-5, relative
to max(|ref|, 1 W), pointwise; status, covered bit and NaN pattern exact).

Measured on an MI355X (each probe test prints its figures before it asserts; DESIGN.md "(c) Oracle and
parity" keeps them):
  probe, random rows    fp64 1.2e-14 (default) / 1.8e-13 (system A), fp32 7.2e-7 / 2.0e-6, no risky point in 20,000;
  probe, planted rows   fp64 1.4e-14 / 1.7e-13, fp32 off the guard bands 5.6e-7 / 3.4e-6; the fp32 chain before the
                        fixup is up to 1.5e-2 / 3.4e-2 off at the flagged points, every one of them flagged;
  world sites, fp32     8.0e-6 at most (a low sun's beam on a vertical panel, airmass 11-12, just above the cut-in,
                        where DISC's Kn_c - Kn cancels and input errors come out 25-50 times larger in the power).

Two defects these tests exposed are fixed with them (tmh_model.h): pv_power_d decided DISC's kt = 0.6 split on
the product form of kt, an ulp off the reference's quotient, so a planted second within two ulps of the split came
out up to 3.3e-2 off; and the per-chain fp32 rows (site_geom_hc, F32) formed GHI_cs, DISC's airmass, Kn_c and 1 / I0h
in fp32, which left the world sites' fp32 power up to 2.2e-5 off (72 seconds of 691,200 past the bar).
"""
import numpy as np
import pytest

import pv_util as U
from test_gpu_parity import _check_vs_oracle, _same, _sim

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


# ------------------------------------------------------------------ 1a
@pytest.mark.parametrize("start", U.WINDOWS_A, ids=["noon", "cut_in", "dusk"])
@pytest.mark.parametrize("path", ["sequential", "time_parallel"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_system_a_vs_oracle(prec, path, start):
    ref = U.ref_a(start)
    sim = _sim(U.N_CHAINS, start, tz=U.TZ_A, mp=U.params_a(), prec=prec, horizon=U.STEPS_A, kernel_path=path)
    assert sim.path == path
    out = sim.run(U.STEPS_A)
    np.testing.assert_array_equal(sim.status(), ref["status"])
    _check_vs_oracle(out, ref, prec)


# ------------------------------------------------------------------ 1b
def _world(run, path, prec, linke):
    start, tz = U.WORLD_RUNS[run]
    sites = (U.world_sites(), U.world_linke() if linke else None)
    sim = _sim(U.N_CHAINS, start, tz=tz, mp=U.world_params(), prec=prec, horizon=U.WORLD_STEPS, kernel_path=path,
               sites=sites)
    assert sim.path == path
    return sim, sim.run(U.WORLD_STEPS, window=U.WORLD_WINDOW)


@pytest.mark.parametrize("run", sorted(U.WORLD_RUNS))
@pytest.mark.parametrize("path,prec,linke", [("time_parallel", "fp64", False), ("time_parallel", "fp32", True),
                                             ("sequential", "fp64", True), ("sequential", "fp32", False)])
def test_world_sites_vs_oracle(path, prec, linke, run):
    ref = U.ref_world(run, linke)
    sim, out = _world(run, path, prec, linke)
    np.testing.assert_array_equal(sim.status(), ref["status"])
    _check_vs_oracle(out, ref, prec)


@pytest.mark.parametrize("run", sorted(U.WORLD_RUNS))
@pytest.mark.parametrize("linke", [True, False])
def test_world_sites_fp32_paths_agree(linke, run):
    """The fp32 cases of the table above, time-parallel == sequential bit for bit (as
    test_c5_slice_time_parallel_equals_sequential_and_oracle on the European grid): the block-night shortcut
    and the hour-angle anchors' rotation must not differ between the two kernels."""
    a, ra = _world(run, "time_parallel", "fp32", linke)
    b, rb = _world(run, "sequential", "fp32", linke)
    np.testing.assert_array_equal(a.status(), b.status())
    for f in ("csi", "covered", "pv", "meter", "residual"):
        assert _same(ra[f], rb[f]), f


# ------------------------------------------------------------------ 2: the probe
@pytest.fixture(scope="module")
def engines():
    """One engine per probe system and its real rows: every 600th second of its day."""
    out = {}
    for name, (mp, start, tz) in U.probe_systems().items():
        sim = _sim(1, start, tz=tz, mp=mp, horizon=86400)
        out[name] = (sim, mp, sim.geometry(0, 86400)[::U.ROW_STRIDE].cpu().numpy().copy())
    return out


def _figures(tag, got, ref, sel=None):
    """Print a probe comparison's figures (fp64 and fp32 maxima, the risky share), return (e64, e32, risky)."""
    e64, e32, risky = U.rel_err(got[:, 0], ref), U.rel_err(got[:, 1], ref), got[:, 2] != 0
    sel = np.ones(len(ref), bool) if sel is None else sel
    held = sel & ~risky
    print(f"\n{tag}: {sel.sum()} points, fp64 max {e64[sel].max():.3e}, fp32 max (not risky) "
          f"{e32[held].max() if held.any() else 0.0:.3e}, fp32 max (risky, before the fixup) "
          f"{e32[sel & risky].max() if (sel & risky).any() else 0.0:.3e}, risky share {risky[sel].mean():.3e}")
    return e64, e32, risky


@pytest.mark.parametrize("name", ["default", "a"])
def test_probe_pv_random_rows(engines, name):
    """Group 1: real rows, 20,000 clear-sky indices uniform in (0, 2.5)."""
    sim, mp, rows = engines[name]
    assert rows.shape == (144, U.ROW) and set(np.unique(rows[:, U.G_DISCOK])) <= {0.0, 1.0}
    pr, pc = U.random_points(rows, seed=20 + len(name))
    ref = U.oracle_points(mp, pr, pc)[0]
    got = sim.probe_pv(pr, pc)
    e64, e32, risky = _figures(f"probe_pv random [{name}]", got, ref)
    assert set(np.unique(got[:, 2])) <= {0.0, 1.0}
    assert e64.max() <= U.TOL64, (e64.max(), pc[e64.argmax()])
    bad = ~risky & (e32 > U.TOL32)
    assert not bad.any(), (bad.sum(), e32[bad].max(), pc[bad][:5])
    assert risky.mean() <= 1e-3, risky.mean()
    assert (ref > 0).mean() > 0.25                          # the comparison is not of zeros


@pytest.mark.parametrize("name", ["default", "a", "c3pos"])
def test_probe_pv_planted_rows(engines, name):
    """Group 2: the clear-sky index, or a field of the row, on each discontinuity and clamp of the chain.
    c3pos (a module with C3 > 0 and C2 = 0): the zero-irradiance rows only, where its vmp is +inf + 0 * -inf."""
    sim, mp, rows = engines[name]
    rows = rows[rows[:, U.G_GHICS] > 0]
    pr, pc, kind = U.planted_points(rows, mp, clip=name == "a")
    if name == "c3pos":
        keep = kind == "ee_zero"
        pr, pc, kind = pr[keep], pc[keep], kind[keep]
    assert 0 < len(pc) <= 100000
    ref, kt, pdc = U.oracle_points(mp, pr, pc)
    got = sim.probe_pv(pr, pc)
    nan = kind == "csi_nan"
    e64, e32, risky = _figures(f"probe_pv planted [{name}]", got, ref, ~nan)
    for kd in sorted(set(kind) - {"csi_nan"}):
        _figures(f"  {kd}", got, ref, kind == kd)
    assert np.isfinite(got[:, :2]).all()
    assert e64.max() <= U.TOL64, (kind[e64.argmax()], e64.max(), pc[e64.argmax()])
    bad = ~nan & ~risky & (e32 > U.TOL32)
    assert not bad.any(), (sorted(set(kind[bad])), bad.sum(), e32[bad].max(), pc[bad][:5])
    if name != "c3pos":
        # the cut-in's guard band (1e-4 of Pso) against the fp32 p_dc error it was sized for (1e-5): every point
        # within 5e-5 of the cut-in must be flagged
        pso = mp.inverter["Pso"]
        must = (kind == "cut_in") & (np.abs(pdc / pso - 1.0) < 5e-5)
        assert must.sum() > 100 and risky[must].all(), (must.sum(), (~risky[must]).sum())
        # a NaN clear-sky index (faulted chains, lanes past the last chain): the fp64 chain gives 0; the fp32
        # chain's min(csi, csi_max) gives csi_max (test_probe_math, probes 10 and 16), so the row's power there
        at_max = np.nonzero(kind == "csi_max")[0][:len(rows)]            # the k = 0 points, row by row
        assert (got[nan, 0] == 0.0).all()
        np.testing.assert_array_equal(got[nan, 1], got[at_max, 1])
        np.testing.assert_array_equal(pc[at_max], rows[:, U.G_CSIMAX])
