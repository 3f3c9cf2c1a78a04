"""The inputs of tests/test_gpu_pv_inputs.py on the oracle alone: each set reaches the part of the
PV chain it is there for, so a kernel that passes the GPU comparison has been through the inverter's
clip, the cut-in, sunrise and sunset, the date line, polar day and night, both DISC regimes and
every planted edge.  No GPU: the C oracle and the library's host side only."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import pv_util as U
from oracle import oracle as O
from tmhpvsim_amd.params import ModelParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1a: a system in which every folded constant shows
def test_system_a_windows_reach_clip_and_cut_in():
    noon, dawn, dusk = (U.ref_a(w) for w in U.WINDOWS_A)
    for r in (noon, dawn, dusk):
        assert (r["status"] == 0).all()
    paco = U.INVERTER_A["Paco"]
    share = (noon["pv"] == paco).mean()
    assert 0.10 <= share <= 0.60, share                    # the clip fires, and not everywhere
    assert noon["pv"].max() == paco and (noon["pv"] > 0).all()
    for r in (dawn, dusk):                                  # the cut-in is crossed in both
        assert (r["pv"] == 0).any() and (r["pv"] > 0).any()
        assert r["pv"].max() < paco
    # the parameters are in effect: same seed and window on the default system
    assert np.abs(noon["pv"] - U.ref_a(U.WINDOWS_A[0], True)["pv"]).max() > 10.0


# (where the constant lives, its key); Pnt is left out: the night tare -|Pnt| is clipped to 0 before any
# output of the oracle (pv_power's .clip(lower=0)), so no trace can show it
SENSITIVE = [("module", "Mbvmp"), ("site", "wind_speed"), ("module", "FD"), ("site", "temp_air"), ("module", "Aimp"),
             ("module", "C1"), ("module", "C3"), ("inverter", "Pso")]


@pytest.mark.parametrize("where,key", SENSITIVE)
def test_system_a_is_sensitive_to_each_folded_constant(where, key):
    """A 1 % change of each constant the host folds into PV64 / PVF moves the oracle's trace by more than 1e-9
    relative (the fp64 bar is 1e-12), so a folding error in any of them shows in the GPU comparison."""
    mp = U.params_a()
    if where == "site":
        mp.site = dataclasses.replace(mp.site, **{key: getattr(mp.site, key) * 1.01})
    else:
        getattr(mp, where)[key] *= 1.01
    worst = 0.0
    for w in U.WINDOWS_A[:2]:                               # noon and the cut-in window
        ref = U.ref_a(w)["pv"]
        got = O.run(mp, 0, U.N_CHAINS, U.STEPS_A, w, tz=U.TZ_A, n_threads=8, outputs=("pv",))["pv"]
        worst = max(worst, U.rel_err(got, ref).max())
    assert worst > 1e-9, (key, worst)


# ------------------------------------------------------------------ 1b: sites around the world
def test_world_sites_layout():
    s = U.world_sites()
    assert s.shape == (128, 8)
    np.testing.assert_array_equal(s[::16, 0], U.WORLD_LATS)             # latitude-major
    np.testing.assert_array_equal(s[:16, 1], U.world_lons())
    assert s[0, 1] == -179.99 and s[15, 1] == 179.99 and s[8, 1] == 0.0
    np.testing.assert_array_equal(s[::16, 2], U.WORLD_ALTS)
    np.testing.assert_array_equal(s[:8, 3], [0.0, 20.0, 48.12, 90.0] * 2)
    np.testing.assert_array_equal(s[:16:4, 4], [0.0, 90.0, 180.0, 270.0])


@pytest.mark.parametrize("run", sorted(U.WORLD_RUNS))
def test_world_runs_reach_every_regime(run):
    """Per run, from orc_geometry at every 60th second (lit: clear-sky GHI > 0): sunrises, sunsets, a latitude
    row in the dark throughout and one lit throughout, lit sites on both sides of the date line."""
    ref = U.ref_world(run, False)
    assert (ref["status"] == 0).all() and (U.ref_world(run, True)["status"] == 0).all()
    lit = U.world_geometry(run, 60)[:, :, U.GEOM16.index("ghi_cs")] > 0
    rise, sset = ~lit[:, 0] & lit[:, -1], lit[:, 0] & ~lit[:, -1]
    assert rise.sum() >= 4 and sset.sum() >= 4, (rise.sum(), sset.sum())
    rows_night, rows_day = (~lit.any(1)).reshape(8, 16).all(1), lit.all(1).reshape(8, 16).all(1)
    assert rows_night.any() and rows_day.any(), (rows_night, rows_day)
    assert (ref["pv"][:, np.repeat(rows_night, 16)] == 0).all()
    lon = U.world_sites()[:, 1]
    seen = lit.any(1) & (ref["pv"] > 0).any(0)
    assert seen[lon == -179.99].any() and seen[lon == 179.99].any()
    # the traces themselves: pv > 0 first or last only (the cut-in makes these fewer than the geometric ones)
    pv = ref["pv"] > 0
    assert (~pv[0] & pv[-1]).sum() >= 4 and (pv[0] & ~pv[-1]).sum() >= 4


def test_world_december_reaches_paco_at_high_sites():
    ref = U.ref_world("december", False)
    at = (ref["pv"] == 250.0).any(0).reshape(8, 16).any(1)
    assert at.any() and (np.asarray(U.WORLD_ALTS)[at] >= 2850.0).all(), at      # the default inverter clips once the site is high


def test_polar_day_row_has_both_disc_regimes():
    run, row = U.POLAR_DAY_ROW
    g = U.world_geometry(run, 1, (row,))
    lit = g[:, :, U.GEOM16.index("ghi_cs")] > 0
    assert lit.all()                                                            # the sun does not set on this row
    ok = g[:, :, U.GEOM16.index("disc_ok")]
    assert (lit & (ok == 0)).sum() >= 1000 and (lit & (ok == 1)).sum() >= 1000


# ------------------------------------------------------------------ 2: the probe's points
def test_orc_pv_row_is_orc_pv():
    mp = U.params_a()
    P = O.make_params(mp)
    cal, utc = O.calendar("2019-06-21 00:00:00", 86400, U.TZ_A)
    for s in range(0, 86400, 3571):
        g = O.geometry(P, utc[s], cal[s, 4], cal[s, 5])
        for csi in (0.0, 0.4, 1.0, 1.7):
            want = O.lib().orc_pv(C.byref(P), int(utc[s]), int(cal[s, 4]), int(cal[s, 5]), csi)
            assert O.pv_row(P, g, csi) == want
            pv, kt, pdc = O.pv_row_parts(P, g[None, :], [csi])
            assert pv[0] == want and 0.0 <= kt[0] <= 1.0


def test_rows_round_trip():
    rows = U.oracle_day_rows("a")
    assert rows.shape == (144, U.ROW)
    g = U.geom16_of(rows)
    np.testing.assert_array_equal(U.geom16_of(U.rows_of(g)), g)
    day = rows[:, U.G_GHICS] > 0
    assert 40 < day.sum() < 144
    np.testing.assert_array_equal(rows[day, U.G_KTC], rows[day, U.G_GHICS] / rows[day, U.G_I0H])


@pytest.mark.parametrize("name", ["default", "a"])
def test_random_points_rarely_sit_on_a_discontinuity(name):
    """The random group's cap on the share of guard-band seconds (1e-3) is met by the reference itself with
    bands twice the kernels' (fp32 guards: |kt - 0.6| < 4e-6, |p_dc - Pso| < 1e-4 Pso): fp64 kt within 8e-6 of
    0.6 or p_dc within 2e-4 Pso of the cut-in.  About 30 % of the points lie above csi_max."""
    mp = U.probe_systems()[name][0]
    rows, csi = U.random_points(U.oracle_day_rows(name), seed=20 + len(name))
    pv, kt, pdc = U.oracle_points(mp, rows, csi)
    pso = mp.inverter["Pso"]
    near = (np.abs(kt - 0.6) < 8e-6) | (np.abs(pdc - pso) < 2e-4 * pso)
    assert near.mean() <= 1e-3, near.mean()
    day = rows[:, U.G_GHICS] > 0
    above = csi[day] > rows[day, U.G_CSIMAX]
    assert 0.15 < above.mean() < 0.45 and (pv[day] > 0).mean() > 0.5
    assert (pv[~day] == 0).all()


@pytest.mark.parametrize("name", ["default", "a"])
def test_planted_points_sit_on_their_edges(name):
    mp = U.probe_systems()[name][0]
    rows = U.oracle_day_rows(name)
    rows = rows[rows[:, U.G_GHICS] > 0]
    pr, pc, kind = U.planted_points(rows, mp, clip=name == "a")
    assert len(pc) <= 100000 and pr.shape == (len(pc), U.ROW)
    pv, kt, pdc = U.oracle_points(mp, pr, pc)
    pso, paco = mp.inverter["Pso"], mp.inverter["Paco"]
    k = kind == "kt_split_unclipped"
    assert (kt[k] <= 0.6).sum() > 50 and (kt[k] > 0.6).sum() > 50 and np.abs(kt[k] - 0.6).max() < 1e-13
    k = kind == "kt_split"                                   # clipped by csi_max on some rows, on the split on the others
    assert (np.abs(kt[k] - 0.6) < 1e-4).sum() > 100 and (kt[k] > 0.6).any() and (kt[k] <= 0.6).any()
    k = kind == "kt_one"                                     # the clamp at 1: on it (1 / ktc lands an ulp either side) and far above
    assert (kt[k] >= 1.0 - 4e-16).all() and (kt[k] == 1.0).sum() >= 2 * len(rows)
    assert (kt[kind == "kt_zero"] == 0.0).all()
    assert (pv[kind == "kt_zero"] == 0.0).all() and (pv[kind == "csi_negative"] == 0.0).all()
    assert (pv[kind == "ee_zero"] == 0.0).all() and (pv[kind == "csi_nan"] == 0.0).all()
    k = kind == "cut_in"
    assert k.sum() > 200 and (pdc[k] < pso).sum() > 100 and (pdc[k] >= pso).sum() > 100
    assert (np.abs(pdc[k] / pso - 1.0) < 5e-5).sum() > 100    # points the guard band must flag
    assert (np.abs(pdc[k] / pso - 1.0) > 2e-4).sum() > 50     # and points it need not
    for kd in ("disc_off", "am_12", "dni_negative", "csi_max"):
        assert (kind == kd).sum() >= len(rows) and np.isfinite(pv[kind == kd]).all()
    if name == "a":
        k = kind == "paco"
        assert (pv[k] == paco).sum() > 50 and (pv[k] < paco).sum() > 50 and (pv[k] > paco * (1 - 1e-3)).all()


def test_c3_positive_module_makes_vmp_nan_at_zero_irradiance():
    mp = U.probe_systems()["c3pos"][0]
    rows = U.oracle_day_rows("c3pos")
    rows = rows[rows[:, U.G_GHICS] > 0].copy()
    rows[:, U.G_F1] = 0.0
    pv, kt, pdc = U.oracle_points(mp, rows, np.full(len(rows), 0.9))
    assert np.isnan(pdc).all() and (pv == 0.0).all()          # vmp = +inf + 0 * -inf: NaN, filled with 0


# ------------------------------------------------------------------ the test hook's host side
def test_probe_pv_is_declared_exported_and_validates():
    from tmhpvsim_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tmhpvsim.h")).read()
    assert "int tmh_probe_pv(struct tmh_engine* eng" in hdr and "#define TMH_ABI_VERSION 1" in hdr
    assert "tmh_probe_pv" in _lib.EXPORTS
    L = _lib.load()
    assert L.tmh_abi_version() == 1
    assert L.tmh_probe_pv(None, None, None, None, 1, None) == -1
    assert b"NULL engine" in L.tmh_last_error()
