"""Night tiles of the single-site expansion (expand_tile's NIGHT instantiation).

A 128-second block whose every four-step group is a night group (the plan's FL_B_NIGHT
mark on the block's first row) runs, in the trace (OUT_TRACE3) and statistics (OUT_STATS)
kernels, a tile that loads the chain's status and fault step only: no samplers, no
descriptor, no segment records, no minute draws, no LDS staging.  The OUT_ANY kernel (any
other combination of outputs) takes no such shortcut, so every test here compares the
shortcut kernels with an OUT_ANY run of the same chains, bit for bit:

  * 200 chains (not a multiple of 64) over three hours across sunrise and across sunset
    (Munich, 2019-09-05): all-night blocks, blocks that straddle the transition, daylight
    blocks and a short last block (10,800 = 84 x 128 + 48); fp32 and fp64; traces and
    statistics (accumulators and histogram);
  * the same window started off the four-step grid, where no block is marked;
  * the plan's marks read back (FL_B_NIGHT on a block's first row): blocks are marked on the
    grid, each of them dark, and none off it -- so the runs above did and did not take the
    shortcut;
  * no PV (every tile of the shortcut kernels is a night tile), on the grid and off it
    (single seconds), again against OUT_ANY;
  * markov cloud cover (chains that fault at construction, in an earlier window, and
    inside a night block): NaN from the fault step on, equal status and equal statistics;
  * two windows, the second all night: the chain state after it is the unshortcut run's
    (the night tile leaves alone what the commit writes back).

Reference: tmhpvsim/pvmodel.py:62-80 (PV is 0 at night), metersim.py:49-51
(meter), pvsim.py:83 (residual).
"""
import functools

import numpy as np
import pytest

from tmhpvsim_amd.params import CC_MARKOV, ModelParams

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TZ = "Europe/Berlin"
N, STEPS = 200, 10800
STARTS = {"sunrise": "2019-09-05 04:45:00", "sunset": "2019-09-05 18:30:00"}
FIELDS = ("pv", "meter", "residual")
ALL5 = ("csi", "covered") + FIELDS
BLOCK = 128
G_FLAGS, FL_NIGHT, FL_B_NIGHT = 3, 8, 128   # tmh_model.h: the geometry row's flags column and its bits


def _sim(n, start, prec, steps, chain0=31000, mp=None):
    from tmhpvsim_amd.engine import BatchedSim
    return BatchedSim(n, start, tz=TZ, params=mp or ModelParams(), precision=prec, chain0=chain0, device="cuda:0",
                      horizon=steps)


def _last(sim):
    return sim.L.tmh_engine_last_expand(sim._eng)


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-12345.0), torch.nan_to_num(b, nan=-12345.0))


def _blocks(pv):
    """per whole 128-step block of a window's pv trace [steps, n] (numpy): dark (every chain 0
    in every second), lit (some chain > 0 in every second), mixed (neither)"""
    nb = pv.shape[0] // BLOCK
    p = np.nan_to_num(pv[:nb * BLOCK], nan=0.0).reshape(nb, BLOCK, -1)
    dark = (p == 0).all(axis=(1, 2))
    lit = (p > 0).any(axis=2).all(axis=1)
    return dark, lit, ~dark & ~lit


def _marks(sim, step0, steps):
    """the plan's flags of the window, per whole block: marked FL_B_NIGHT / every second FL_NIGHT"""
    fl = sim.geometry(step0, steps)[:, G_FLAGS].cpu().numpy().astype(np.int64)
    nb = steps // BLOCK
    marked = (fl[0:nb * BLOCK:BLOCK] & FL_B_NIGHT) != 0
    night = ((fl[:nb * BLOCK] & FL_NIGHT) != 0).reshape(nb, BLOCK).all(axis=1)
    assert not (fl[nb * BLOCK:] & FL_B_NIGHT).any() and not (fl.reshape(-1)[np.arange(len(fl)) % BLOCK != 0] & FL_B_NIGHT).any()
    return marked, night


@functools.lru_cache(maxsize=None)
def _runs(prec, which, lead, with_pv=True):
    """The window `which` (after a first window of `lead` steps, 0 for none) run three ways on
    the same chains: the three traces (OUT_TRACE3), statistics alone (OUT_STATS), and all five
    fields with statistics beside them (OUT_ANY).  Computed once, never modified."""
    from tmhpvsim_amd import _lib
    f64 = _lib.OUT_FP64 if prec == "fp64" else 0
    mp = ModelParams(with_pv=with_pv)
    sims = [_sim(N, STARTS[which], prec, lead + STEPS, mp=mp) for _ in range(3)]
    t3, st, any_ = sims
    st.enable_stats()
    any_.enable_stats()
    if lead:
        for s in sims:
            s.run(lead, trace=ALL5 if s is any_ else FIELDS if s is t3 else (), window=lead)
        st.enable_stats()     # the window's own statistics
        any_.enable_stats()
    o3 = t3.run(STEPS, trace=FIELDS, window=STEPS)
    assert _last(t3) == _lib.OUT_TRACE3 | f64
    st.run(STEPS, trace=(), window=STEPS)
    assert _last(st) == _lib.OUT_STATS | f64
    o5 = any_.run(STEPS, trace=ALL5, window=STEPS)
    assert _last(any_) == _lib.OUT_ANY | f64
    marked, night = _marks(t3, lead, STEPS)
    torch.cuda.synchronize()
    return dict(t3=t3, st=st, any=any_, o3=o3, o5=o5, marked=marked, night=night)


def _check(r):
    for f in FIELDS:
        assert _same(r["o3"][f], r["o5"][f]), f
    for k in ("t3", "st"):
        np.testing.assert_array_equal(r[k].status(), r["any"].status())
        assert torch.equal(r[k].state, r["any"].state), k
    assert torch.equal(r["st"].hist, r["any"].hist)
    assert _same(r["st"].chain_acc, r["any"].chain_acc)
    assert int(r["st"].hist.sum()) > 0


@pytest.mark.parametrize("which", list(STARTS))
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_night_tiles_equal_any(prec, which):
    """Traces and statistics of the shortcut kernels == the OUT_ANY run, over a window that
    holds all-night blocks, blocks straddling the transition and daylight blocks."""
    r = _runs(prec, which, 0)
    dark, lit, mixed = _blocks(r["o5"]["pv"].double().cpu().numpy())
    assert dark.sum() >= 10 and lit.sum() >= 10 and mixed.any(), (dark.sum(), lit.sum(), mixed.sum())
    assert (dark[0] and lit[-1]) if which == "sunrise" else (lit[0] and dark[-1])
    # the plan marked all-night blocks, and only such: these runs took the shortcut
    assert r["marked"].sum() >= 10 and r["night"][r["marked"]].all()
    assert dark[r["marked"]].all() and not r["marked"][lit].any()
    _check(r)


@pytest.mark.parametrize("which", list(STARTS))
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_window_off_the_grid_equals_any(prec, which):
    """The same window after a first one of 1,001 steps: it starts off the four-step grid,
    so the plan marks no block and no tile may take the shortcut."""
    r = _runs(prec, which, 1001)
    dark, lit, _ = _blocks(r["o5"]["pv"].double().cpu().numpy())
    assert dark.any() and lit.any()
    assert r["night"].sum() >= 10 and not r["marked"].any()   # all-night blocks, none marked
    _check(r)


@pytest.mark.parametrize("lead", [0, 1001])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_no_pv_equals_any(prec, lead):
    """Without PV every tile of the trace and statistics kernels is a night tile, marked or not:
    across sunrise on the grid (four-second groups, the short last block's single seconds) and
    off it (single seconds throughout), traces and statistics equal the OUT_ANY run's."""
    r = _runs(prec, "sunrise", lead, False)
    assert float(torch.nan_to_num(r["o5"]["pv"]).abs().max()) == 0.0
    assert not r["night"].all() and float(torch.nan_to_num(r["o5"]["meter"]).abs().max()) > 0.0
    _check(r)


@functools.lru_cache(maxsize=None)
def _fault_runs(prec):
    """markov cloud cover, 3,000 chains from 03:30: a first window of two hours, then the hour
    to 06:30, both before sunrise (the oracle has chains 5000.. fault at steps 6315 and 6388,
    in the first window, and at 8502, 8967, 9218 and 9395, in the second); traces by
    OUT_TRACE3 and by OUT_ANY."""
    n, start, wins = 3000, "2019-09-05 03:30:00", (7200, 3600)
    mp = ModelParams(cc_mode=CC_MARKOV)
    a, b, s = (_sim(n, start, prec, sum(wins), chain0=5000, mp=mp) for _ in range(3))
    b.enable_stats()   # statistics beside the traces (OUT_ANY) and alone (OUT_STATS), over both windows
    s.enable_stats()
    outs = []
    for w in wins:
        status0 = b.status()
        oa = a.run(w, trace=FIELDS, window=w)
        ob = b.run(w, trace=ALL5, window=w)
        s.run(w, trace=(), window=w)
        torch.cuda.synchronize()
        outs.append((oa, ob, status0))
    return a, b, outs, s


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_faulted_chains_in_night_tiles(prec):
    """Chains that faulted at construction or in the first window emit NaN throughout the
    second; a chain that faults inside a night block of the second window emits NaN from its
    fault step on; the same bits and the same status as the OUT_ANY run."""
    a, b, outs, s = _fault_runs(prec)
    assert torch.equal(s.hist, b.hist) and _same(s.chain_acc, b.chain_acc)   # statistics stop at the fault step alike
    np.testing.assert_array_equal(s.status(), b.status())
    for oa, ob, _ in outs:
        for f in FIELDS:
            assert _same(oa[f], ob[f]), f
    np.testing.assert_array_equal(a.status(), b.status())
    assert torch.equal(a.state, b.state)
    (_, o1, s0), (o2a, o2, s1) = outs
    assert (s0 != 0).sum() >= 10                   # faulted at construction
    assert ((s1 != 0) & (s0 == 0)).sum() >= 1      # faulted in the first window
    pv = o2["pv"].double().cpu().numpy()
    bad = np.isnan(o2a["meter"].double().cpu().numpy())
    assert bad[:, s1 != 0].all()
    dark, _, _ = _blocks(pv)
    first = np.where(bad.any(axis=0) & ~bad[0], np.argmax(bad, axis=0), -1)   # fault step inside the window
    hit = [int(j) for j in first if j >= 0 and dark[min(j // BLOCK, len(dark) - 1)] and j % BLOCK]
    assert hit, "the test needs a chain that faults inside an all-night block"
    for j in hit:   # NaN from the fault step on, numbers before it
        c = int(np.argmax(first == j))
        assert bad[j:, c].all() and not bad[:j, c].any()


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_state_after_a_night_window(prec):
    """Two windows from 18:30, the second (21:30-22:30) all night: traces of both windows
    and the chain state after them equal the OUT_ANY run's."""
    wins = (10800, 3600)
    a, b = (_sim(N, STARTS["sunset"], prec, sum(wins)) for _ in range(2))
    for i, w in enumerate(wins):
        oa = a.run(w, trace=FIELDS, window=w)
        ob = b.run(w, trace=ALL5, window=w)
        torch.cuda.synchronize()
        for f in FIELDS:
            assert _same(oa[f], ob[f]), (i, f)
        if i == 1:
            assert float(torch.nan_to_num(ob["pv"]).abs().max()) == 0.0
        assert torch.equal(a.state, b.state), i
