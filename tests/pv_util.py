"""Inputs of the PV-chain tests, shared by tests/test_pv_inputs_cpu.py (the oracle alone) and
tests/test_gpu_pv_inputs.py (the kernels against the oracle).

Three sets of inputs, each chosen so that a part of the PV half the default Munich system
never reaches is in play:

  * SYSTEM_A: a module, an inverter and a site in which every host-folded constant of the chain
    (PV64 / PVF in tmh_engine_create) changes the result -- Mbvmp != 0, wind != 0, FD != 1,
    B0 != 1, C0 + C1 != 1, air temperature != 20 C -- and whose inverter clips at noon;
  * world_sites(): 128 sites over both hemispheres, the date line, both polar circles, four
    tilts, four azimuths and altitudes up to 4,000 m, one per chain (tmh_set_sites);
  * planted_points(): geometry rows with the clear-sky index, or a field of the row, placed on
    each discontinuity and clamp of the chain, for the probe of the chain itself
    (tmh_probe_pv against orc_pv_row).

References are computed once per process (functools.lru_cache) and must not be modified.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from tmhpvsim_amd.params import LINKE_DEFAULT, MODULE_DEFAULT, ModelParams, Site

N_CHAINS = 128

# ------------------------------------------------------------------ a system in which every folded constant shows
MODULE_A = dict(MODULE_DEFAULT, FD=0.93, Mbvmp=0.035, Bvmpo=-0.16, Aimp=0.00045, C0=0.985, C1=0.021, C2=0.27, C3=-6.2,
                N=1.32, Cells_in_Series=72.0, Impo=8.6, Vmpo=36.9, temp_a=-3.56, temp_b=-0.075, temp_deltaT=2.0,
                B0=0.998, A0=0.92)
INVERTER_A = dict(Paco=285.0, Pdco=285.0 * 1.042, Vdco=38.0, Pso=2.9, C0=-6.3e-5, C1=-2.1e-4, C2=8.1e-4, C3=-0.021,
                  Pnt=0.11)
SEED_A, TZ_A, STEPS_A = 0xBEEF, "Europe/Berlin", 3600
WINDOWS_A = ("2019-06-21 12:30:00", "2019-06-21 05:15:00", "2019-06-21 20:30:00")   # noon, cut-in, dusk


def site_a():
    return Site(48.12, 11.60, altitude=520.0, tilt=30.0, surface_azimuth=205.0, albedo=0.4, temp_air=-5.0,
                wind_speed=3.5)


def params_a(**kw):
    return ModelParams(seed=SEED_A, site=site_a(), module=dict(MODULE_A), inverter=dict(INVERTER_A), **kw)


@functools.lru_cache(maxsize=None)
def ref_a(start, default=False):
    """The oracle's run of a SYSTEM_A window (default: the same seed and window on the default system)."""
    mp = ModelParams(seed=SEED_A) if default else params_a()
    return O.run(mp, 0, N_CHAINS, STEPS_A, start, tz=TZ_A, n_threads=8)


# ------------------------------------------------------------------ sites around the world
WORLD_LATS = (-78.0, -66.0, -33.9, -23.44, 0.0, 23.44, 48.12, 69.65)
WORLD_ALTS = (34.0, 0.0, 50.0, 2850.0, 2850.0, 4000.0, 520.0, 10.0)      # per latitude row
WORLD_TILTS, WORLD_AZIMUTHS = (0.0, 20.0, 48.12, 90.0), (0.0, 90.0, 180.0, 270.0)
WORLD_RUNS = {"june": ("2019-06-21 02:30:00", "Europe/Berlin"), "december": ("2019-12-21 09:00:00", None)}
WORLD_STEPS, WORLD_WINDOW, WORLD_SEED = 5400, 2000, 0x51E
# The polar-day row: 66 S in December.  The sun never sets there (lowest elevation 66 + 23.44 - 90 = -0.56 deg,
# inside the refraction band) and spends hours under DISC's zenith > 87 deg cut.  At 69.65 N in June and 78 S in
# December it stays above 3 deg (3.09 and 11.4 deg), so DISC is valid throughout.
POLAR_DAY_ROW = ("december", 1)


def world_lons():
    lon = np.linspace(-180.0, 157.5, 16)
    lon[0], lon[-1] = -179.99, 179.99
    return lon


def world_sites():
    """[128, 8] in Site.as_array() order, latitude-major: 8 latitudes x 16 longitudes."""
    lon = world_lons()
    s = np.empty((8, 16, 8))
    s[..., 0] = np.asarray(WORLD_LATS)[:, None]
    s[..., 1] = lon[None, :]
    s[..., 2] = np.asarray(WORLD_ALTS)[:, None]
    s[..., 3] = np.asarray([WORLD_TILTS[j % 4] for j in range(16)])[None, :]
    s[..., 4] = np.asarray([WORLD_AZIMUTHS[j // 4] for j in range(16)])[None, :]
    s[..., 5], s[..., 6], s[..., 7] = 0.25, 20.0, 0.0
    return s.reshape(N_CHAINS, 8)


def world_linke():
    """Per-site monthly Linke turbidity, as tests/test_gpu_parity.py::test_site_grid_vs_oracle draws it."""
    return np.asarray(LINKE_DEFAULT)[None, :] * (0.8 + 0.4 * np.random.default_rng(3).random((N_CHAINS, 1)))


def world_params():
    return ModelParams(seed=WORLD_SEED)


@functools.lru_cache(maxsize=None)
def ref_world(run, linke):
    start, tz = WORLD_RUNS[run]
    return O.run(world_params(), 0, N_CHAINS, WORLD_STEPS, start, tz=tz, n_threads=8,
                 sites=(world_sites(), world_linke() if linke else None))


def site_params(mp, site, linke=None):
    """OrcParams of mp with columns 0-5 of a site row (and its Linke turbidity) in place of mp.site's."""
    P = O.make_params(mp)
    for i in range(6):
        P.site[i] = float(site[i])
    if linke is not None:
        for i in range(12):
            P.linke[i] = float(linke[i])
    return P


@functools.lru_cache(maxsize=None)
def world_geometry(run, every=1, rows=None):
    """orc_geometry of every world site (or of the latitude rows given, a tuple) at every `every`-th second of
    a run and at its last: [n_sites, n_seconds, 16] (geom_t's order, GEOM16)."""
    start, tz = WORLD_RUNS[run]
    cal, utc = O.calendar(start, WORLD_STEPS, tz)
    sites, mp = world_sites(), world_params()
    pick = range(N_CHAINS) if rows is None else [16 * r + j for r in rows for j in range(16)]
    secs = list(range(0, WORLD_STEPS, every))
    if secs[-1] != WORLD_STEPS - 1:
        secs.append(WORLD_STEPS - 1)
    out = np.empty((len(pick), len(secs), 16))
    f = O.lib().orc_geometry
    for a, c in enumerate(pick):
        P = site_params(mp, sites[c])
        ref = C.byref(P)
        for b, s in enumerate(secs):
            f(ref, int(utc[s]), int(cal[s, 4]), int(cal[s, 5]), out[a, b].ctypes.data_as(C.c_void_p))
    return out


# ------------------------------------------------------------------ geometry rows: the table's layout and the oracle's
# fields of a table row (tmh_model.h, G_*)
G_FLAGS, G_COSZ, G_CSIMAX, G_GHICS, G_I0H, G_I0, G_KNC, G_AM, G_F2, G_RB, G_DNIEXTRA = 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
G_TERM2, G_GFAC, G_COSAOI, G_F1, G_DISCOK, G_KTC, G_RDNIX, ROW = 14, 15, 16, 17, 18, 19, 20, 22
# the oracle's geom_t: cosz csi_max ghi_cs i0h i0 knc am disc_ok cos_zen rb dni_extra term2 gfac cos_aoi f1 f2
GEOM16 = ("cosz", "csi_max", "ghi_cs", "i0h", "i0", "knc", "am", "disc_ok", "cos_zen", "rb", "dni_extra", "term2",
          "gfac", "cos_aoi", "f1", "f2")
GEOM16_COLS = [G_COSZ, G_CSIMAX, G_GHICS, G_I0H, G_I0, G_KNC, G_AM, G_DISCOK, G_COSZ, G_RB, G_DNIEXTRA, G_TERM2,
               G_GFAC, G_COSAOI, G_F1, G_F2]


def geom16_of(rows):
    """Table rows [..., 22] -> the oracle's geom_t [..., 16]."""
    return np.ascontiguousarray(np.asarray(rows)[..., GEOM16_COLS])


def rows_of(geom16):
    """The oracle's geom_t [n, 16] -> table rows [n, 22] (clock fractions and flags 0; cos_zen is cosz)."""
    g = np.asarray(geom16)
    rows = np.zeros(g.shape[:-1] + (ROW,))
    for k, col in enumerate(GEOM16_COLS):
        if k != 8:
            rows[..., col] = g[..., k]
    return derive(rows)


def derive(rows):
    """Recompute the derived fields of (planted) rows in place: G_KTC = GHI_cs / I0h, G_RDNIX = 1 / dni_extra."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rows[..., G_KTC] = rows[..., G_GHICS] / rows[..., G_I0H]
        rows[..., G_RDNIX] = 1.0 / rows[..., G_DNIEXTRA]
    return rows


# the engines whose rows the probe takes: name -> (params, the day, tz)
ZERO_MODULE = dict(MODULE_DEFAULT, C3=8.0, C2=0.0)     # Ee = 0 gives vmp = +inf + 0 * -inf = NaN


def probe_systems():
    return {"default": (ModelParams(), "2019-09-05 00:00:00", "Europe/Berlin"),
            "a": (params_a(), "2019-06-21 00:00:00", TZ_A),
            "c3pos": (ModelParams(module=dict(ZERO_MODULE)), "2019-09-05 00:00:00", "Europe/Berlin")}


ROW_STRIDE = 600


@functools.lru_cache(maxsize=None)
def oracle_day_rows(name):
    """Every 600th second of a probe system's day as table rows [144, 22], from orc_geometry."""
    mp, start, tz = probe_systems()[name]
    cal, utc = O.calendar(start, 86400, tz)
    P = O.make_params(mp)
    g = np.stack([O.geometry(P, utc[s], cal[s, 4], cal[s, 5]) for s in range(0, 86400, ROW_STRIDE)])
    return rows_of(g)


N_RANDOM = 20000


def random_points(rows, seed):
    """Group 1: N_RANDOM points, point k on row k mod len(rows) with csi uniform in (0, 2.5)."""
    rng = np.random.default_rng(seed)
    csi = rng.uniform(0.0, 2.5, N_RANDOM)
    return np.ascontiguousarray(rows[np.arange(N_RANDOM) % len(rows)]), csi


def _ulps(x, k):
    """x stepped by k units in the last place (x > 0 finite)."""
    return (np.asarray(x, dtype=np.float64).view(np.int64) + np.int64(k)).view(np.float64)


def _bisect(f, lo, hi, iters=80):
    """Per element the smallest hi' and largest lo' in [lo, hi] with f(lo') False, f(hi') True
    (f monotone enough: False at lo, True at hi); returns (lo', hi') adjacent to ~1 ulp."""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        t = f(mid)
        hi = np.where(t, mid, hi)
        lo = np.where(t, lo, mid)
    return lo, hi


REL_STEPS = (1e-7, 1e-6, 1e-5, 1e-4, 1e-3)


def planted_points(rows, mp, clip=False):
    """Group 2: the planted points of one system on its daylight rows (`rows`: table rows [n, 22] with
    ghi_cs > 0; `mp`: the system, for the bisections on the oracle).  Returns (rows [m, 22], csi [m],
    kind [m]) with kind the name of the edge each point sits on.  clip: also the inverter's Paco crossing."""
    P = O.make_params(mp)
    rows = np.asarray(rows)
    assert (rows[:, G_GHICS] > 0).all()
    out_r, out_c, out_k = [], [], []

    def add(kind, r, c):
        r = np.atleast_2d(r)
        c = np.broadcast_to(np.asarray(c, dtype=np.float64), (len(r),))
        out_r.append(derive(r.copy()))
        out_c.append(c.copy())
        out_k.extend([kind] * len(r))

    ktc = rows[:, G_GHICS] / rows[:, G_I0H]
    c06 = 0.6 / ktc                                       # kt = csi ktc = 0.6 (to an ulp)
    for k in (0, 1, -1, 2, -2, 64, -64):
        add("kt_split", rows, _ulps(c06, k))
    for rel in (1e-6, -1e-6, 1e-5, -1e-5):
        add("kt_split", rows, c06 * (1.0 + rel))
    high = rows.copy()                                    # csi_max planted high: the split and the kt clamps unclipped
    high[:, G_CSIMAX] = np.inf
    for k in (0, 1, -1, 2, -2, 64, -64):
        add("kt_split_unclipped", high, _ulps(c06, k))
    add("kt_one", high, 1.0 / ktc)
    add("kt_one", high, _ulps(1.0 / ktc, 4))
    add("kt_one", high, 3.0 / ktc)
    add("kt_zero", rows, 0.0)
    add("csi_negative", rows, -0.25)
    for k in (0, 1, -1):
        add("csi_max", rows, _ulps(rows[:, G_CSIMAX], k))
    for c in (0.3, 0.75, 1.0, 1.3):
        r = rows.copy()
        r[:, G_DISCOK] = 0.0
        add("disc_off", r, c)
        r = rows.copy()
        r[:, G_AM] = 12.0
        add("am_12", r, c)
        r = rows.copy()
        r[:, G_KNC] = 0.02                                # below DISC's Kn at every kt: dni < 0
        add("dni_negative", r, c)
        r = rows.copy()
        r[:, G_F1] = 0.0                                  # Ee = 0: log = -inf
        add("ee_zero", r, c)

    def parts(c, r=rows):
        return O.pv_row_parts(P, geom16_of(r), c)

    pso, paco = float(mp.inverter["Pso"]), float(mp.inverter["Paco"])
    top = np.minimum(rows[:, G_CSIMAX], 2.5)
    zero = np.zeros(len(rows))
    ok = parts(top)[2] > pso                              # the rows on which the cut-in is crossed at all
    if ok.any():
        sub = rows[ok]
        # the crossing itself to an ulp; the points step away from it by 1e-7 and more (at the crossing's two
        # ends an fp64 chain that rounds differently from the oracle by an ulp may sit on either side)
        lo, hi = _bisect(lambda c: parts(c, sub)[2] >= pso, zero[ok], top[ok])
        for rel in REL_STEPS:
            add("cut_in", sub, hi * (1.0 + rel))
            add("cut_in", sub, lo * (1.0 - rel))
    if clip:
        ok = parts(top)[0] >= paco
        if ok.any():
            sub = rows[ok]
            lo, hi = _bisect(lambda c: parts(c, sub)[0] >= paco, zero[ok], top[ok])
            for k in (0, 1, 2, 64):
                add("paco", sub, _ulps(hi, k))
                add("paco", sub, _ulps(lo, -k))
            for rel in (1e-6, 1e-4):
                add("paco", sub, hi * (1.0 + rel))
                add("paco", sub, lo * (1.0 - rel))
    add("csi_nan", rows, np.nan)
    return np.concatenate(out_r), np.concatenate(out_c), np.asarray(out_k)


def oracle_points(mp, rows, csi):
    """(pv, kt, p_dc) of the oracle on table rows and clear-sky indices."""
    return O.pv_row_parts(O.make_params(mp), geom16_of(rows), csi)


# fp32 contract of a second (DESIGN.md "Parity"): within 1e-5 of the fp64 oracle relative to max(|ref|, 1 W),
# or flagged risky and recomputed in fp64; the fp64 chain within 1e-12
TOL64, TOL32 = 1e-12, 1e-5


def rel_err(got, ref):
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
