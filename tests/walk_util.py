"""Planted-state reference for the cloud-segment walk (host only).

The walk (segments_kernel, and next_cloud on the sequential path) restates
CloudCoverBinary.next_cloud (cloud_cover_binary.py:80-107).  The tests that use this
module plant a binary state into a constructed batch, run a short window on the GPU and
compare with the host shim tmhpvsim_amd.cloud_cover_binary.CloudCoverBinary (pinned draw
for draw to the reference by tests/golden/shims.npz) started from the same state:

  * keyed_lengths / Lengths: the unscaled candidate lengths pow(alpha + delta u, expo)
    of (chain, call, try), u from the keyed Philox stream the kernels draw from.  The
    power is numpy's, or the device's own (engine.probe 17) -- the one operation of a
    call that is not IEEE-exact; every other one is an fp64 add, multiply, divide or
    compare, so with the device's powers the comparison is bit for bit;
  * run_reference: one shim per chain, second by second, with the reference's per-second
    update_parameters (clearskyindexmodel.py:113-136);
  * search_equal: the ulp searches that build exact ties and exact equalities;
  * build_cases / check_edges: the case table and the predicates that show each case
    reaches the edge it is named for, according to the reference alone.
"""
from __future__ import annotations

import datetime as dt
import math

import numpy as np

from oracle.philox import TAG_CLOUD, keyed_uniform
from tmhpvsim_amd import cloud_cover_binary as ccb

ALPHA, DELTA, EXPO = ccb._ALPHA, ccb._DELTA, 1 / (1 - ccb._BETA)
CAP = 512                 # TMH_SIGMA_CAP
SEED = 0x5EED
START = dt.datetime(2019, 9, 5, 10, 0, 5)   # naive clock; no hour or day boundary in the window
N_STEPS = 3500
SNAPS = (100, 300, 1200)  # the reference also keeps each chain's state after this many steps (100: after the
                          # first call alone for the chains planted at wind 1, whose segments last 105 s or more)
N_CALLS = 640             # calls per chain whose tries 0 and 1 are drawn up front
CAND_CAP = N_STEPS // 150 + 32     # try-0 candidate table rows of the window (cand_cap)


def row_cap(n_steps):
    return (n_steps // 135 + 16 + 15) & ~15   # segment records per chain row of a window (seg_cap)


ROW_CAP = row_cap(N_STEPS)
OVF_CHUNK = 256           # records per overflow pool chunk


def pool_chunks(n):
    return n // 16 + 8


# ------------------------------------------------------------------ candidate lengths
def numpy_power(arg):
    return arg ** EXPO


def keyed_lengths(seed, chain, call, tries, power=numpy_power):
    """Unscaled candidate lengths x of try `tries` of next_cloud call `call` of `chain`
    (broadcast): x = power(alpha + delta u), u the keyed uniform (call, TAG_CLOUD, try >> 1,
    try & 1).  power: numpy's `** expo`, or a callable giving the device's (probe 17)."""
    t = np.asarray(tries, dtype=np.int64)
    u = keyed_uniform(seed, chain, call, TAG_CLOUD, t >> 1, t & 1)
    return np.asarray(power(np.ascontiguousarray(ALPHA + DELTA * u)), dtype=np.float64)


class Lengths:
    """x(chain, call, try): tries 0 and 1 of the first n_calls calls of every chain drawn at
    once, later tries (and calls) on demand, all 40 tries of a call together."""

    def __init__(self, seed, n_chains, n_calls=N_CALLS, power=numpy_power):
        self.seed, self.power = seed, power
        ch = np.arange(n_chains)[:, None, None]
        ca = np.arange(n_calls)[None, :, None]
        self.x01 = keyed_lengths(seed, ch, ca, np.arange(2)[None, None, :], power)
        self.later = {}

    def x(self, chain, call, t):
        if t < 2 and call < self.x01.shape[1] and chain < self.x01.shape[0]:
            return self.x01[chain, call, t]
        key = (chain, call)
        if key not in self.later:
            self.later[key] = keyed_lengths(self.seed, chain, call, np.arange(40), self.power)
        return self.later[key][t]


# ------------------------------------------------------------------ clock and parameters
def fractions(start, step):
    """min / hour / day fraction of `step` seconds after start (clearskyindexmodel.py:114-116)."""
    t = start + dt.timedelta(seconds=step)
    min_fraction = t.second / 60
    hour_fraction = (t.minute + min_fraction) / 60
    day_fraction = (t.hour + hour_fraction) / 24
    return min_fraction, hour_fraction, day_fraction


def interpolate(before, after, fraction):
    return fraction * after + (1 - fraction) * before      # clearskyindexmodel.py:39-40


def params_at(plant, start, step):
    """(hourly cloud cover, wind speed) update_parameters receives at `step`."""
    _, hf, df = fractions(start, step)
    return interpolate(plant["cc_b"], plant["cc_a"], hf), interpolate(plant["ws_b"], plant["ws_a"], df)


def first_call(plant, start=START):
    """(h, f, ws) of a call at step 0: the capped cover, 1 / h - 1 and the wind speed."""
    hh, ws = params_at(plant, start, 0)
    h = min(hh, 0.95)
    with np.errstate(divide="ignore"):
        return h, 1 / h - 1, ws


def make_plant(name, sc, sl, cc=1.0, ws=1.0, cl=10.0, clr=5.0, ncalls=1, **expect):
    """One chain's planted state.  sec = ceil(cl + clr) - 1 puts the first call on step 0."""
    cc_b, cc_a = cc if isinstance(cc, tuple) else (cc, cc)
    ws_b, ws_a = ws if isinstance(ws, tuple) else (ws, ws)
    return dict(name=name, sc=np.asarray(sc, dtype=np.float64), sl=np.asarray(sl, dtype=np.float64),
                cc_b=np.float64(cc_b), cc_a=np.float64(cc_a), ws_b=np.float64(ws_b), ws_a=np.float64(ws_a),
                cl=float(cl), clr=float(clr), sec=int(math.ceil(cl + clr)) - 1, ncalls=int(ncalls), expect=expect)


# ------------------------------------------------------------------ the reference
class SigmaOverflow(Exception):
    """A call's new sigma arrays would exceed TMH_SIGMA_CAP (status 3; no reference analogue)."""


def overflows(length):
    return length > CAP      # last + 2 > TMH_SIGMA_CAP


def _state(shim, status, ctx):
    return dict(status=status, sec=int(shim.sec), cl=float(np.ravel(shim.cloud_length)[0]), clr=float(shim.clear_length),
                sc=np.array(shim.sigma_cloud, dtype=np.float64), sl=np.array(shim.sigma_clear, dtype=np.float64),
                ncalls=ctx["next_call"])


def _run_one(chain, p, fr, ctx, n_steps, shim_cls):
    shim = object.__new__(shim_cls)     # the planted state instead of the constructor's
    shim.sigma_cloud, shim.sigma_clear = p["sc"].copy(), p["sl"].copy()
    shim.cloud_length, shim.clear_length, shim.sec = np.array([p["cl"]]), np.float64(p["clr"]), p["sec"]
    ctx.update(chain=chain, next_call=p["ncalls"], call=None, tries=0)
    inner, calls = shim.next_cloud, []

    def counted(recurse=False):
        if not recurse:
            ctx.update(call=ctx["next_call"], tries=0)
            ctx["next_call"] += 1
            calls.append(dict(step=ctx["step"], call=ctx["call"], L0=len(shim.sigma_cloud), tries=0, last=-1))
        try:
            out = inner(recurse)
        finally:
            calls[-1]["tries"] = ctx["tries"]
        if not recurse:
            calls[-1]["last"] = len(shim.sigma_cloud) - 2
            if overflows(len(shim.sigma_cloud)):
                raise SigmaOverflow()
        return out

    shim.next_cloud = counted
    cov = np.full(n_steps, 255, dtype=np.uint8)
    status, fault, snaps = 0, -1, {}
    with np.errstate(divide="ignore", invalid="ignore"):    # a cover of 0.0: 1 / h = inf
        for s in range(n_steps):
            _, hf, df = fr[s]
            ctx["step"] = s
            shim.update_parameters(interpolate(p["cc_b"], p["cc_a"], hf), interpolate(p["ws_b"], p["ws_a"], df))
            try:
                cov[s] = next(shim)
            except AssertionError:
                status, fault = 2, s
                break
            except SigmaOverflow:
                status, fault = 3, s
                break
            finally:
                if s + 1 in SNAPS:
                    snaps[s + 1] = _state(shim, status, ctx)
    for k in SNAPS:      # a chain that faulted before: its state at the fault
        snaps.setdefault(k, _state(shim, status, ctx))
    return dict(covered=cov, fault=fault, calls=calls, snaps=snaps, **_state(shim, status, ctx))


def run_reference(plants, start, n_steps, lengths, chains=None, uniforms_seed=None, shim_cls=ccb.CloudCoverBinary):
    """The shim from each chain's planted state over n_steps seconds.  Per chain: the covered
    trace (255 from a fault on), the final sec / cl / clr / sigma arrays / call count, the
    status (0, 2 the shim's AssertionError, 3 the sigma capacity), the fault step, one record
    per next_cloud call (step, call number, length before, tries, last), and `snaps`, the
    same state fields after SNAPS steps.

    The shim module's random_cloudlength_in_s is replaced for the run: it returns x / ws from
    `lengths` for the chain's current call and try (numpy's global stream is not used).
    chains: the plants' chain ids (default: their positions).  uniforms_seed (the check of
    this loop itself): leave the shim's own function in place and feed it the same keyed
    uniforms through np.random.random instead."""
    fr = [fractions(start, s) for s in range(n_steps)]
    chains = range(len(plants)) if chains is None else chains
    ctx = {}

    def patched(windspeed, shape=(1,)):
        x = lengths.x(ctx["chain"], ctx["call"], ctx["tries"])
        ctx["tries"] += 1
        return np.array([x / windspeed])

    def uniforms(shape=None):
        t = ctx["tries"]
        ctx["tries"] += 1
        return np.full(shape, keyed_uniform(uniforms_seed, ctx["chain"], ctx["call"], TAG_CLOUD, t >> 1, t & 1))

    target, name, repl = (ccb, "random_cloudlength_in_s", patched) if uniforms_seed is None else (np.random, "random", uniforms)
    saved = getattr(target, name)
    setattr(target, name, repl)
    try:
        return [_run_one(c, p, fr, ctx, n_steps, shim_cls) for c, p in zip(chains, plants)]
    finally:
        setattr(target, name, saved)


def candidate(plant, x, start=START):
    """Try arithmetic of a call at step 0 with unscaled length x, on the planted arrays, as
    CloudCoverBinary._candidate computes it: (cl, span, new clear - old clear, ok)."""
    h, f, ws = first_call(plant, start)
    with np.errstate(divide="ignore", invalid="ignore"):
        cl = x / ws
        cum_cloud = plant["sc"] + cl
        cum_clear = cum_cloud * (1 / h - 1)
        span = cum_cloud + cum_clear
        dl = cum_clear - plant["sl"]
        return cl, span, dl, (dl > 0) & (span < 5400)


# ------------------------------------------------------------------ ulp searches
def _tot(cl, f, sc):
    nsc = cl + sc
    return nsc + f * nsc


def _walk(x0, width):
    yield x0
    up = dn = x0
    for _ in range(width):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        yield up
        yield dn


def search_equal(kind, cl, f, arg=None, width=300):
    """Exact equalities of a try with cloud length cl and clear factor f, by walking
    np.nextafter over `width` neighbours each way; None when there is none.
      "symmetric", D: (sc_a, sc_b), tot_a != tot_b and |tot_a - 3600| == |tot_b - 3600|
                      bit for bit (tot_a about 3600 - D);
      "tot", T:       sc with tot == T exactly (5400.0: the strict span bound);
      "clear", sc:    sl with nsl - sl == 0.0 exactly."""
    cl, f = np.float64(cl), np.float64(f)
    if kind == "clear":
        sl = f * (cl + np.float64(arg))
        return sl if f * (cl + np.float64(arg)) - sl == 0.0 else None
    if kind == "tot":
        T = np.float64(arg)
        for sc in _walk(T / (1 + f) - cl, width):
            if _tot(cl, f, sc) == T:
                return sc
        return None
    assert kind == "symmetric"
    sc_a = np.float64(3600.0 - arg) / (1 + f) - cl
    ta = _tot(cl, f, sc_a)
    T = 3600.0 + (3600.0 - ta)
    if not (ta < 3600.0 and T - 3600.0 == 3600.0 - ta):
        return None
    sc_b = search_equal("tot", cl, f, T, width)
    if sc_b is None or abs(_tot(cl, f, sc_b) - 3600.0) != abs(ta - 3600.0):
        return None
    return sc_a, sc_b


# ------------------------------------------------------------------ the case table
DUP_PAIRS = [(3, 7), (3, 11), (3, 19),      # the same group lane in different chunks, G = 4, 8, 16
             (3, 9),                         # different lanes of one chunk
             (60, 70), (30, 40),             # across the register / global boundary (64; 32 in the TP walk)
             (100, 300)]                     # both in the global row
SYM_PAIRS = [(2, 5), (5, 2), (40, 70), (70, 40)]
LAST_TOP = [3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 509, 510]
COVERS = [1.0, 0.95, 0.9499999, 0.5, 0.2]


def build_cases(lengths):
    """The planted batch: [plant], slot = chain id.  The cases are laid out so that the
    slots of one kind are spread over the batch (stride 37), i.e. wavefronts mix them."""
    makers = []      # (name, function of the chain id -> plant)

    def nice_call(chain):    # the first call number whose try-0 length is 100 .. 2,000 m: cl at wind 1
        for k in range(1, N_CALLS):
            if 100.0 <= lengths.x(chain, k, 0) <= 2000.0:
                return k
        raise AssertionError("no call with a short try-0 length")

    def base(chain, cc=1.0, ws=1.0):
        k = nice_call(chain)
        h, f, w = first_call(make_plant("", [], [], cc=cc, ws=ws))
        return k, lengths.x(chain, k, 0) / w, h, f

    def structured(chain, L, last):
        """Entry `last` nearest one hour; the others 2.5 s apart below it, 3.5 s and more above
        (so the runner-up is unique too); every entry possible."""
        k, cl, h, f = base(chain)
        idx = np.arange(L)
        sc = 3600.0 * h - cl + 2.5 * (idx - last) + (idx > last) * 1.0
        return k, cl, f, sc

    def add(name, fn):
        makers.append((name, fn))

    def dup(i, j):
        def fn(chain):
            k, cl, f, sc = structured(chain, j + 4, i)
            sc[j] = sc[i]
            return make_plant(f"dup{i}_{j}", sc, f * sc, ncalls=k, kind="dup", pair=(i, j), last=i)
        return fn

    def sym(i, j):
        def fn(chain):
            k, cl, h, f = base(chain)
            for D in range(10, 26):
                got = search_equal("symmetric", cl, f, float(D))
                if got is not None:
                    break
            L = max(i, j) + 4
            sc = 3600.0 * h - cl - 60.0 - 2.5 * np.arange(L)      # the others: 60 s and more below
            found = got is not None
            if found:
                sc[i], sc[j] = got        # the lower tot at i, the upper at j
            return make_plant(f"sym{i}_{j}", sc, f * sc, ncalls=k, kind="sym", pair=(i, j), last=min(i, j), found=found)
        return fn

    def span_only(chain):
        k, cl, h, f = base(chain)
        s = search_equal("tot", cl, f, 5400.0)
        found = s is not None
        s = s if found else 5400.0 * h - cl
        sc = np.array([s + 50.0, s, s + 100.0])
        return make_plant("span5400_only", sc, f * sc, ncalls=k, kind="span_only", at=1, found=found)

    def span_pair(order):
        def fn(chain):
            k, cl, h, f = base(chain)
            s = search_equal("tot", cl, f, 5400.0)
            found = s is not None
            s = s if found else 5400.0 * h - cl
            lo = s
            for _ in range(8):                   # the lower neighbour: the next sc whose span is below 5400
                lo = np.nextafter(lo, -np.inf)
                if _tot(cl, f, lo) < 5400.0:
                    break
            sc = np.array([s, lo] if order == 0 else [lo, s])
            return make_plant(f"span5400_pair{order}", sc, f * sc, ncalls=k, kind="span_pair", at=order,
                              last=1 - order, found=found)
        return fn

    def clear_eq(shift):
        def fn(chain):
            k, cl, f, sc = structured(chain, 6, 2)
            sl = f * sc
            z = search_equal("clear", cl, f, sc[2])
            sl[2] = z if shift == 0 else np.nextafter(z, -np.inf if shift < 0 else np.inf)
            return make_plant(f"clear0_{'eq' if shift == 0 else 'below' if shift < 0 else 'above'}", sc, sl, ncalls=k,
                              kind="clear", at=2, shift=shift)
        return fn

    def clear_big(L, i):
        def fn(chain):
            k, cl, f, sc = structured(chain, L, i)
            sl = f * sc
            sl[i - 1:i + 2] = 1e6
            return make_plant(f"clear_big{L}_{i}", sc, sl, ncalls=k, kind="clear_big", at=(i - 1, i, i + 1))
        return fn

    def place(L, last, **kw):
        def fn(chain):
            k, cl, f, sc = structured(chain, L, last)
            return make_plant(f"L{L}_last{last}", sc, f * sc, ncalls=k, kind="place", L=L, last=last, **kw)
        return fn

    def ladder(name, cc, ws, sc, **kw):
        def fn(chain):
            p = make_plant(name, sc, sc, cc=cc, ws=ws, kind="ladder", **kw)
            _, f, _ = first_call(p)
            if np.isfinite(f):      # (a cover of 0.0: any clear lengths do, every span is infinite)
                p["sl"] = f * p["sc"]
            return p
        return fn

    def fresh(name, cc, ws, **kw):
        """The state reset_sigma leaves: 300 (k + 1) s of cloud, k < int(12 h), clear time in proportion."""
        def fn(chain):
            p = make_plant(name, [], [], cc=cc, ws=ws, kind="fresh", **kw)
            h, f, _ = first_call(p)
            p["sc"] = 300.0 * np.arange(1, int(h * 12) + 1, dtype=np.float64)
            p["sl"] = f * p["sc"]
            return p
        return fn

    for rep in range(2):
        for i, j in DUP_PAIRS:
            add("dup", dup(i, j))
        for i, j in SYM_PAIRS:
            add("sym", sym(i, j))
        add("span", span_only)
        add("span", span_pair(0))
        add("span", span_pair(1))
        for shift in (0, -1, 1):
            add("clear", clear_eq(shift))
        add("clear", clear_big(8, 4))
        add("clear", clear_big(80, 64))
    for L in (1, 2, 65, 512):
        add("place", place(L, 0))
    for L in LAST_TOP:
        add("place", place(L, L - 1))
    for last in (31, 32, 33, 62, 63, 64):         # the register / global boundary of either walk
        add("place", place(200, last))
    for L, last in ((100, 15), (100, 16), (40, 4)):
        add("place", place(L, last))
    add("place", place(512, 511, status=3))
    add("place", place(512, 510))
    far = 5130.0 + 10.0 * np.arange(6)
    for rep in range(2):
        add("ladder", ladder("reject20_reset", 1.0, 1.0, far, tries_min=21, status=0))
        add("ladder", ladder("reject40_wind", 1.0, 0.01, far, tries_min=40, status=2))
        add("ladder", ladder("cover005", 0.05, 1.0, 300.0 * np.arange(1, 4), tries_min=40, status=2))
        add("ladder", ladder("cover0", 0.0, 1.0, 300.0 * np.arange(1, 4), tries_min=40, status=2))
    for rep in range(4):
        for cc in COVERS:
            add("cover", fresh(f"cover{cc}", cc, 3.0))
    add("cover", fresh("cover_fall", (1.0, 0.9), (2.0, 6.0)))      # crosses the 0.95 cap inside the window
    add("cover", fresh("cover_rise", (0.9, 1.0), (6.0, 2.0)))
    for ws in (40.0, 200.0, 1000.0, 200.0, 40.0, 200.0, 1000.0):
        add("wind", fresh(f"wind{int(ws)}", 1.0, ws, wind=ws))

    n = len(makers)
    assert n % 64 and n % 37      # a partly live last wavefront; the stride visits every slot
    plants = [None] * n
    for i, (group, fn) in enumerate(makers):
        slot = i * 37 % n
        plants[slot] = fn(slot)
        plants[slot]["group"] = group
    return plants


def check_edges(plants, ref, lengths):
    """Every case reaches the edge it is named for, by the reference alone (asserts)."""
    n = len(plants)
    for c, (p, r) in enumerate(zip(plants, ref)):
        e, name = p["expect"], f"chain {c} {p['name']}"
        assert r["calls"] and r["calls"][0]["step"] == 0 and r["calls"][0]["call"] == p["ncalls"], name
        first = r["calls"][0]
        cl, span, dl, ok = candidate(p, lengths.x(c, p["ncalls"], 0))
        d = np.abs(span - 3600)
        kind = e["kind"]
        if kind in ("dup", "sym", "span_pair", "clear", "clear_big", "place"):      # SNAPS[0] sees the first call alone
            assert len(r["calls"]) == 1 or r["calls"][1]["step"] >= SNAPS[0], name
        if kind in ("dup", "sym"):
            i, j = e["pair"]
            assert e.get("found", True), f"{name}: no exact symmetric tie found"
            assert ok[i] and ok[j] and d[i] == d[j] and d[i] == d[ok].min() and (d[ok] == d[i]).sum() == 2, name
            assert (span[i] == span[j]) == (kind == "dup"), name
            assert first["tries"] == 1 and first["last"] == min(i, j) == e["last"], name
        elif kind == "span_only":
            assert e["found"] and span[e["at"]] == 5400.0 and not ok.any() and (dl > 0).all(), name
            assert first["tries"] >= 2, name
        elif kind == "span_pair":
            a = e["at"]
            assert e["found"] and span[a] == 5400.0 and span[1 - a] < 5400.0 and not ok[a] and ok[1 - a], name
            assert first["tries"] == 1 and first["last"] == 1 - a, name
        elif kind == "clear":
            a = e["at"]
            assert d[a] == d.min() and (span < 5400).all(), name
            if e["shift"] == 0:
                assert dl[a] == 0.0 and not ok[a] and first["last"] != a, name
            elif e["shift"] < 0:
                assert 0.0 < dl[a] < 1e-12 and first["last"] == a, name
            else:
                assert -1e-12 < dl[a] < 0.0 and not ok[a] and first["last"] != a, name
        elif kind == "clear_big":
            at = list(e["at"])
            assert (span < 5400).all() and not ok[at].any() and ok.sum() == len(ok) - 3, name
            assert d[at[1]] == d.min() and first["last"] not in at and first["tries"] == 1, name
        elif kind == "place":
            assert ok.all() and first["L0"] == e["L"] and first["last"] == e["last"] and first["tries"] == 1, name
            rest = np.delete(d, e["last"])
            assert len(rest) == 0 or rest.min() - d[e["last"]] >= 2.0, name
            if e.get("status") == 3:
                assert r["status"] == 3 and r["fault"] == 0, name
            else:
                assert r["fault"] != 0, name
        elif kind == "ladder":
            assert first["tries"] >= e["tries_min"], name
            if e["status"] == 2:
                assert r["status"] == 2 and r["fault"] == 0 and first["tries"] == 40, name
            else:
                assert r["fault"] != 0 and first["last"] >= 0 and first["L0"] == 6, name

    def by(key):
        return [r for p, r in zip(plants, ref) if p["name"] == key]

    # mixed covers: at the cap and below it, all walking without an early fault
    assert len({p["name"] for p in plants if p["group"] == "cover"}) == len(COVERS) + 2
    assert all(len(r["calls"]) >= 3 for r in by("cover1.0") + by("cover0.95") + by("cover0.9499999"))
    # wind 200: growth call by call through every chunk boundary, past the candidate table and the record row
    grown = {c["L0"] for r in by("wind200") for c in r["calls"] if c["last"] == c["L0"] - 1}
    assert set(range(11, 130)) <= grown, sorted(set(range(11, 130)) - grown)
    assert max(len(r["calls"]) for r in by("wind200")) > max(CAND_CAP, ROW_CAP)
    assert max(c["L0"] for r in by("wind200") for c in r["calls"]) > 128
    for r in by("wind1000"):       # reaches the capacity, then status 3
        assert r["status"] == 3 and max(c["L0"] for c in r["calls"]) == CAP and len(r["calls"]) > 500
    # the overflow pool never runs short: chains that leave their record row, and the chunks they take
    for steps in SNAPS + (N_STEPS,):
        records = [1 + sum(c["step"] < steps for c in r["calls"]) for r in ref]
        leave = [k - row_cap(steps) for k in records if k > row_cap(steps)]
        assert 0 < len(leave) <= n // 16 and sum(-(-k // OVF_CHUNK) for k in leave) <= pool_chunks(n), (steps, leave)
    assert sum(r["status"] == 3 for r in ref) >= 2 and sum(r["status"] == 2 for r in ref) >= 6
    # retries and sigma lengths the statistics of a constructed batch almost never reach
    assert max(c["L0"] for r in ref for c in r["calls"]) == CAP
