"""The range-end inputs without a GPU (range_util): conditions that the reference loops alone meet on the oracle's
traces, so the GPU tests that share these inputs (test_gpu_range_ends) are known to run at the ends of the ranges
tmhpvsim.h documents -- input D's int32 half-wave partials one quantum under 2^31, the corner recipe's 40-bit states
of charge, 17-bit kd and parameters at both ends of every range, the clamp pattern, and the sweeps at 16 variants.
Every floor is a condition on an input, not a measurement of the code under test."""
import numpy as np
import pytest

from dispatch_sweep_util import rolled
from dispatch_util import identities, run, soc_changes
from range_util import (C_LEAD, C_STEPS, CAP_TOP, CORNER_OBSERVED, D_HALF_WAVE, D_N, D_Q, D_STEPS, D_WINDOWS, INT64_MAX,
                        INT64_MIN, assert_corners_bite, assert_d_bites, c60_oracle, clip, corner_counts, corners, d_oracle,
                        d_params, poison, poison_soc, rolled_corners)
from series_util import A_N
from storage_util import a60_oracle
from sweep_util import variants
from test_battery_cpu import _loop, _slice_chains
from tmhpvsim_amd import battery, demand, dispatch, registers, series

IV = 900
PARAMS, SOC0 = corners()


def _a():
    ref = a60_oracle()
    return ref["pv"], ref["meter"], ref["covered"], ref["status"]


@pytest.fixture(scope="module")
def a_corner():
    """dispatch.from_traces and dispatch_util.run of A's 60-module traces at the corner recipe."""
    pv, meter, cov, status = _a()
    return dispatch.from_traces(pv, meter, cov, IV, params=PARAMS, soc0=SOC0), run(pv, meter, cov, IV, PARAMS, SOC0), status


def test_input_d_sits_one_quantum_under_the_int32_bound():
    """Conditions on D, observed on the oracle's traces: 3,523 (step, half-wave) pairs whose 32 chains' q(pv) sum to
    exactly 32 x 67,107,840 = 2^31 - 32,768; 94.3 % of the ok chain-seconds exactly at Paco; 24 chains dead at
    construction and none that faults inside the window.  The floors: 1,000 pairs, a share of 0.9, 10 chains."""
    mp = d_params()
    assert mp.inverter["Paco"] == 16383.75 < series.MAX_W == 16384.0
    assert int(series.quantize(np.float32(16383.75))) == int(series.quantize(16383.75)) == D_Q
    assert D_HALF_WAVE == 32 * D_Q == 2147450880 == (1 << 31) - 32768
    assert D_N % 32 == 8 and sum(D_WINDOWS) == D_STEPS and D_WINDOWS[0] % 4 and D_WINDOWS[0] % 128
    ref = d_oracle()
    c = assert_d_bites(ref["pv"], ref["covered"], ref["status"])
    print(c)
    ok = ref["covered"] != 255
    assert float(np.nanmax(ref["pv"])) == 16383.75 and int(series.quantize(ref["pv"])[ok].max()) == D_Q
    # a signed 32-bit partial of one more lane at Paco would wrap: the input leaves no slack
    assert D_HALF_WAVE + D_Q > (1 << 31) - 1
    # the registers' and the demand table's export side reaches q(Paco) - q(meter) per second
    rg = registers.from_traces(ref["pv"], ref["meter"], ref["covered"], IV)
    dm = demand.from_traces(ref["pv"], ref["meter"], ref["covered"], 7)
    np.testing.assert_array_equal(rg[:, 4] - rg[:, 5], rg[:, 1] - rg[:, 0])
    peak = demand.unpack(dm[:, 7])[0]
    d = np.where(ok, series.quantize(ref["pv"]) - series.quantize(ref["meter"]), 0)
    assert int(peak.max()) == int(d.max()) > D_Q - (9000 << 12) and int(peak.max()) <= D_Q


def test_corner_recipe_values():
    assert PARAMS.shape == (9, A_N) and PARAMS.dtype == np.int64 and SOC0.shape == (A_N,) and SOC0.dtype == np.int64
    dispatch.check_params(PARAMS)
    battery.check_params(PARAMS[:6])
    for row, (lo, hi) in enumerate(dispatch.RANGES):                       # both ends of every row occur
        assert int(PARAMS[row].min()) == lo and int(PARAMS[row].max()) == hi, row
        assert len(set(PARAMS[row].tolist())) == 4, row
    assert ((SOC0 >= 0) & (SOC0 <= PARAMS[0])).all()
    assert ((SOC0 == CAP_TOP) & (PARAMS[0] == CAP_TOP)).any() and ((SOC0 == 0) & (PARAMS[0] == CAP_TOP)).any()
    kd = battery._recip(PARAMS[4])
    assert int(kd.max()) == 1 << 17 and int(kd.min()) == 1 << 16 and ((kd > 1 << 16) & (kd < 1 << 17)).any()
    par, soc = rolled_corners(16, 1300)
    assert par.shape == (16, 9, 1300) and soc.shape == (16, 1300)
    np.testing.assert_array_equal(par[0, :, :A_N], PARAMS)
    np.testing.assert_array_equal(par[3, :, :A_N], np.roll(np.tile(PARAMS, (1, 2))[:, :1300], 3 * 37, axis=1)[:, :A_N])
    dispatch.check_sweep_params(par)


def test_corner_recipe_two_derivations_and_its_counts(a_corner):
    """dispatch.from_traces equals dispatch_util.run at the corner recipe, and the input bites.  Observed on the oracle's
    60-module traces of A at interval_s = 900 (the floors are half of each): 1,336 cells with SoC >= 2^39, 60 chains
    with ed = 2^15 that discharged, 109 with ec = 2^15 that charged, 248 with L = 0 that curtailed, 136 with Pc = 2^27
    that charged, 69,683 partial fills, 20,946 partial empties, 73,259 seconds that curtail while a full battery clips
    the charge, 592 chains with a loss; the maximum SoC is 2^40 - 1 exactly."""
    (want, end), (got, gend, ev), status = a_corner
    for col in range(13):
        np.testing.assert_array_equal(want[:, col], got[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(end, gend)
    counts = corner_counts(want, ev, PARAMS)
    print(counts)
    assert_corners_bite(counts)
    assert set(CORNER_OBSERVED) < set(counts)
    identities(want, PARAMS)
    soc_changes(want, SOC0, end)
    dead = status == 1
    assert dead.any() and not want[:, :, dead].any() and (end[dead] == SOC0[dead]).all()


def test_corner_battery_against_the_scalar_loop():
    """battery.from_traces against test_battery_cpu's loop over Python integers on its slice of chains (dead, faulting
    and live ones), with the corner recipe's batteries: 40-bit capacities, 2^27 power limits and drains, kd = 2^17."""
    pv, meter, cov, status = _a()
    chains = _slice_chains(cov, status)
    assert len(chains) >= 12
    sub = [a[:, chains] for a in (pv, meter, cov)]
    par, x0 = PARAMS[:6, chains], SOC0[chains]
    got, end = battery.from_traces(*sub, IV, params=par, soc0=x0)
    want, wend = _loop(*sub, IV, 0, par, x0)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(end, wend)


def test_corner_recipe_has_teeth(a_corner, monkeypatch):
    """The expected table notices the errors the recipe is for: a state of charge cut to 32 bits before it is packed
    changes at least 100 cells; a kd kept in 16 bits (2^17 and 2^16 become 0, the values between lose their top bit)
    changes the table too."""
    (want, end), _, _ = a_corner
    pv, meter, cov, _ = _a()
    cut = (want[:, 8] >> 40 << 40) | (want[:, 8] & 0xFFFFFFFF)
    assert int((cut != want[:, 8]).sum()) >= 100
    stored = battery._stored
    monkeypatch.setattr(battery, "_stored", lambda a, ec, kd: stored(a, ec, kd & 0xFFFF))
    bad, bend = dispatch.from_traces(pv, meter, cov, IV, params=PARAMS, soc0=SOC0)
    monkeypatch.undo()
    cells = int((bad != want).sum())
    print("cells changed by a 16-bit kd:", cells, "chains:", int((bad != want).any(axis=(0, 1)).sum()))
    assert cells >= 100 and (bend != end).any()
    live = (bad != want).any(axis=(0, 1))
    assert (PARAMS[4, live] == 1 << 15).any() and (PARAMS[4, live] == 1 << 16).any()   # both ends of ed among them


@pytest.mark.parametrize("stagger", [False, True], ids=["pattern", "staggered"])
@pytest.mark.parametrize("kind", ["battery", "dispatch"])
def test_clamp_pattern(kind, stagger):
    """The pattern puts hi + 1, -1, INT64_MAX and INT64_MIN into every row; the loops refuse such parameters
    (check_params), so the expectation of the GPU test is the loop at the clipped ones -- which differs from the loop at
    the valid parameters the pattern was written over, so a kernel that ignored the overwritten values would fail.
    Under (i + row) % 5 rows five apart get the same case, so a threshold is below 0 only where its power limit clamps
    to 0 and a missing lower clamp of Tc or Td could not show; the staggered pattern has chains where it would, and the
    loop at Tc = -1 in place of 0 differs there."""
    mod = battery if kind == "battery" else dispatch
    rows = len(mod.RANGES)
    n = 320
    pv, meter, cov = c60_oracle(n)
    valid, soc_valid = rolled_corners(1, n)
    valid, soc_valid = valid[0, :rows], soc_valid[0]
    bad = poison(valid, mod.RANGES, stagger=stagger)
    for row, (lo, hi) in enumerate(mod.RANGES):
        case = (np.arange(n) + row + (row // 5 if stagger else 0)) % 5
        assert sorted(set(bad[row, case != 4].tolist())) == [INT64_MIN, -1, hi + 1, INT64_MAX]
        np.testing.assert_array_equal(bad[row, case == 4], valid[row, case == 4])
    ok = clip(bad, mod.RANGES)
    if kind == "dispatch":
        shows = (bad[6] == -1) & (ok[1] > 0) & (ok[0] > 0)                   # Tc below 0 at a battery that can charge
        assert shows.any() == stagger
        if stagger:
            off = ok.copy()
            off[6, shows] = 1                                               # (a stand-in inside the range for a Tc let through)
            other, _ = mod.from_traces(pv, meter, cov, 60, origin=C_LEAD, params=off, soc0=np.clip(poison_soc(soc_valid, ok[0], rows), 0, ok[0]))
            ref, _ = mod.from_traces(pv, meter, cov, 60, origin=C_LEAD, params=ok, soc0=np.clip(poison_soc(soc_valid, ok[0], rows), 0, ok[0]))
            assert (other != ref).any(axis=(0, 1))[shows].any()
    mod.check_params(ok)
    soc_bad = poison_soc(soc_valid, ok[0], rows)
    assert (soc_bad > ok[0]).any() and (soc_bad < 0).any()
    with pytest.raises(ValueError):
        mod.from_traces(pv, meter, cov, 60, origin=C_LEAD, params=bad, soc0=soc_bad)
    want, end = mod.from_traces(pv, meter, cov, 60, origin=C_LEAD, params=ok, soc0=np.clip(soc_bad, 0, ok[0]))
    plain, pend = mod.from_traces(pv, meter, cov, 60, origin=C_LEAD, params=valid, soc0=soc_valid)
    assert want.shape == plain.shape == (-(-(C_STEPS + C_LEAD) // 60), len(mod.COLUMNS), n)
    differ = (want != plain).any(axis=(0, 1))
    print(kind, "chains whose table the pattern changes:", int(differ.sum()), "of", n)
    assert int(differ.sum()) >= n // 4 and (end != pend).any()
    assert ((end >= 0) & (end <= ok[0])).all()


def test_sixteen_variants_differ():
    """The sweeps' maximum: sixteen rolled variants pass check_sweep_params, a seventeenth does not, and on input C
    every variant's table differs from every other's (so a group loop that wrote one group's variants into another's
    tables would be seen)."""
    n = 320
    pv, meter, cov = c60_oracle(n)
    par, soc0 = rolled(16, n, "C")
    with pytest.raises(ValueError):
        dispatch.check_sweep_params(rolled(17, n, "C")[0])
    with pytest.raises(ValueError):
        battery.check_sweep_params(variants(17, n)[0])
    table, end = dispatch.sweep_from_traces(pv, meter, cov, 60, origin=C_LEAD, params=par, soc0=soc0)
    bpar, bsoc = variants(16, n)
    btable, bend = battery.sweep_from_traces(pv, meter, cov, 60, origin=C_LEAD, params=bpar, soc0=bsoc)
    for t in (table, btable):
        for u in range(16):
            for v in range(u + 1, 16):
                assert (t[u, :, 4:] != t[v, :, 4:]).any(), (u, v)
            np.testing.assert_array_equal(t[u, :, :4], t[0, :, :4])
    for v in (0, 3, 4, 8, 15):                                                     # the sweep's loop is the kind's, variant by variant
        want, wend = dispatch.from_traces(pv, meter, cov, 60, origin=C_LEAD, params=par[v], soc0=soc0[v])
        np.testing.assert_array_equal(table[v], want)
        np.testing.assert_array_equal(end[v], wend)
        want, wend = battery.from_traces(pv, meter, cov, 60, origin=C_LEAD, params=bpar[v], soc0=bsoc[v])
        np.testing.assert_array_equal(btable[v], want)
        np.testing.assert_array_equal(bend[v], wend)
