"""The cloud-segment walk against the reference from planted states.

Every other test of segments_kernel / next_cloud starts from the constructor's state and
lets the model's statistics decide what is exercised.  Here a binary state is planted into
a constructed batch (BatchedSim.state_field views are writable), a window of 3,500 s with
no hour or day boundary is run, and every chain is compared with the host shim
CloudCoverBinary started from the same state (walk_util.run_reference; the shim is pinned
to the reference draw for draw by tests/golden/shims.npz, cloud_cover_binary.py:80-107).

The reference takes the one operation of a call that is not IEEE-exact, the cloud-length
power, from the device itself (engine.probe 17, pinned to numpy at 1e-14 in
test_probe_math); everything else in a call is an fp64 add, multiply, divide or compare and
the library is built with -ffp-contract=off, so status, the covered trace and the state
are compared exactly, the lengths and sigma arrays bit for bit.

The case table (walk_util.build_cases; tests/test_walk_reference_cpu.py shows on the host
that each case reaches its edge and that a walk with one rule broken fails on it): exact
ties of |tot - 3600| -- duplicate entries and symmetric pairs, within a lane, across lanes,
chunks and the register / global boundary --, tot == 5400 and a clear difference of 0
exactly, the chosen `last` at every chunk boundary of every lane width, lengths up to 512
and TMH_CHAIN_SIGMA_OVERFLOW past it, the retry ladder (20 rejections and a reset; 40 and
TMH_CHAIN_ASSERT_BINARY; an empty reset at covers 0.05 and 0.0), covers at and below the
0.95 cap side by side in a wavefront, and wind speeds whose arrays grow entry by entry past
the try-0 candidate table and the record row into the overflow pool.
"""
import os

import numpy as np
import pytest

import walk_util as W
from tmhpvsim_amd.params import ModelParams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# id: kernel path, lanes per chain (0: the default), chains per row, rows in wind order, the
# 8-lane throughput walk (32 register entries), precision
VARIANTS = {
    "sequential": ("sequential", 0, 0, 1, 0, "fp64"),
    "tp16_cpr1": ("time_parallel", 16, 1, 1, 0, "fp64"),
    "tp16_cpr3": ("time_parallel", 16, 3, 1, 0, "fp64"),
    "tp8_cpr1": ("time_parallel", 8, 1, 1, 0, "fp64"),
    "tp8_cpr3": ("time_parallel", 8, 3, 0, 0, "fp64"),
    "tp4_cpr1": ("time_parallel", 4, 1, 0, 0, "fp64"),
    "tp4_cpr3": ("time_parallel", 4, 3, 1, 0, "fp64"),
    "tp8_throughput": ("time_parallel", 8, 1, 1, 1, "fp64"),
    "tp4_cpr1_fp32": ("time_parallel", 4, 1, 1, 0, "fp32"),
}


def _device_power(arg):
    from tmhpvsim_amd.engine import probe
    return probe(17, W.EXPO, arg, device="cuda:0")


@pytest.fixture(scope="module")
def planted():
    """The case table and its reference, once, with the device's own cloud-length powers."""
    lengths = W.Lengths(W.SEED, 128, power=_device_power)
    plants = W.build_cases(lengths)
    assert 100 <= len(plants) <= 130 and len(plants) % 64
    ref = W.run_reference(plants, W.START, W.N_STEPS, lengths)
    host = W.Lengths(W.SEED, 128).x01
    rel = np.abs(lengths.x01 - host) / host
    print(f"device pow_d against numpy over {host.size} planted-stream uniforms: max rel {rel.max():.3e}, "
          f"{(rel > 0).sum()} differ; {len(lengths.later)} calls drew tries past the second")
    return plants, ref, lengths


def _sim(variant, plants):
    """A fresh sim of the variant with the planted binary state."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    path, lanes, cpr, order, tp, prec = VARIANTS[variant]
    n = len(plants)
    env = {"TMH_WALK_TP_ROWS": "1" if tp else "4294967295"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = BatchedSim(n, W.START, tz=None, params=ModelParams(seed=W.SEED, with_pv=False), precision=prec,
                       device="cuda:0", horizon=W.N_STEPS, kernel_path=path)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert s.path == path
    s.built_ok = s.status() == 0      # chains whose constructor drew valid samplers (their csi is finite)
    if path == "time_parallel":
        L = _lib.load()
        _lib.check(L.tmh_set_walk_lanes(s._eng, lanes))
        _lib.check(L.tmh_set_walk_chains_per_row(s._eng, cpr))
        _lib.check(L.tmh_set_walk_order(s._eng, order))
    sc = np.zeros((n, W.CAP))
    sl = np.zeros((n, W.CAP))
    for c, p in enumerate(plants):
        sc[c, :len(p["sc"])] = p["sc"]
        sl[c, :len(p["sl"])] = p["sl"]
    col = lambda key, dt: np.array([p[key] for p in plants], dtype=dt)
    fields = {"sb_cc": col("cc_b", np.float64), "sa_cc": col("cc_a", np.float64),
              "sb_ws": col("ws_b", np.float64), "sa_ws": col("ws_a", np.float64),
              "cloud_length": col("cl", np.float64), "clear_length": col("clr", np.float64),
              "sec": col("sec", np.int32), "sigma_len": np.array([len(p["sc"]) for p in plants], dtype=np.int32),
              "sigma_cloud": sc, "sigma_clear": sl, "ncalls": col("ncalls", np.int32),
              "status": np.zeros(n, dtype=np.int32)}
    for name, arr in fields.items():
        view = s.state_field(name)
        view.copy_(torch.as_tensor(arr, device=view.device).view_as(view))
    torch.cuda.synchronize()
    return s


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _state_mismatches(sim, plants, want, what):
    """Chains whose device state differs from the reference's `want` states: status exact; for
    status-0 chains sec, sigma_len and ncalls exact, the lengths and sigma arrays bit for bit."""
    g = {k: sim.state_field(k).cpu().numpy() for k in ("status", "sec", "sigma_len", "ncalls", "cloud_length",
                                                       "clear_length", "sigma_cloud", "sigma_clear")}
    bad = []
    for c, (p, w) in enumerate(zip(plants, want)):
        diff = []
        if int(g["status"][c]) != w["status"]:
            diff.append(f"status {int(g['status'][c])} != {w['status']}")
        elif w["status"] == 0:      # a faulted chain's state is frozen, not defined
            L = len(w["sc"])
            for key, val in (("sec", w["sec"]), ("sigma_len", L), ("ncalls", w["ncalls"])):
                if int(g[key][c]) != val:
                    diff.append(f"{key} {int(g[key][c])} != {val}")
            for key, val in (("cloud_length", w["cl"]), ("clear_length", w["clr"])):
                if _bits(g[key][c]) != _bits(val):
                    diff.append(f"{key} {float(g[key][c])!r} != {val!r}")
            if int(g["sigma_len"][c]) == L:
                for key, val in (("sigma_cloud", w["sc"]), ("sigma_clear", w["sl"])):
                    ne = np.nonzero(_bits(g[key][c, :L]) != _bits(val))[0]
                    if len(ne):
                        diff.append(f"{key}[{ne[0]}] {float(g[key][c, ne[0]])!r} != {float(val[ne[0]])!r} ({len(ne)} of {L})")
        if diff:
            bad.append(f"{what}: chain {c} {p['name']}: " + "; ".join(diff))
    return bad


def test_planted_reference_reaches_its_edges(planted):
    """With the device's powers the case table still reaches every edge (the predicates of
    tests/test_walk_reference_cpu.py: the exact ties and equalities are searched with the
    device's candidate lengths)."""
    plants, ref, lengths = planted
    W.check_edges(plants, ref, lengths)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_walk_planted(planted, variant):
    """Status, covered trace and window-end binary state of every planted chain equal the
    reference's, on the sequential path and on the time-parallel path at every lane width,
    with queued rows, in wind and in chain order, in the 8-lane throughput walk and with the
    fp32 expansion.  Fresh sims given 100, 300 and 1,200 steps pin the state after the first
    call alone and while the windy chains' arrays are long (later calls shorten them again)."""
    plants, ref, _ = planted
    n = len(plants)
    bad = []
    for k in W.SNAPS:
        s = _sim(variant, plants)
        out = s.run(k, trace=("covered",))
        torch.cuda.synchronize()
        bad += _state_mismatches(s, plants, [r["snaps"][k] for r in ref], f"after {k} steps")
        cov = out["covered"].cpu().numpy()
        for c, r in enumerate(ref):
            if not np.array_equal(cov[:, c], r["covered"][:k]):
                bad.append(f"after {k} steps: chain {c} {plants[c]['name']}: covered differs from step "
                           f"{int(np.argmax(cov[:, c] != r['covered'][:k]))}")
    s = _sim(variant, plants)
    out = s.run(W.N_STEPS, trace=("csi", "covered"))
    torch.cuda.synchronize()
    status = s.status()
    assert not (status == 5).any(), "the record pool ran short (TMH_CHAIN_SEGMENT_OVERFLOW)"
    bad += _state_mismatches(s, plants, ref, "window end")
    cov = out["covered"].cpu().numpy()
    csi = out["csi"].double().cpu().numpy()
    assert cov.shape == (W.N_STEPS, n)
    for c, r in enumerate(ref):
        name = f"window: chain {c} {plants[c]['name']}"
        if not np.array_equal(cov[:, c], r["covered"]):      # the reference's trace is 255 from the fault step on
            bad.append(f"{name}: covered differs from step {int(np.argmax(cov[:, c] != r['covered']))} "
                       f"(reference status {r['status']} at {r['fault']})")
        f = r["fault"] if r["status"] else W.N_STEPS
        if not np.isnan(csi[f:, c]).all() or (s.built_ok[c] and np.isnan(csi[:f, c]).any()):
            bad.append(f"{name}: csi is not NaN exactly from the fault step {f} on")
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:40])
