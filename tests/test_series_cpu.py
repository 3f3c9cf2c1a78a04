"""The fleet series without a GPU: the contract in numpy (tmhpvsim_amd.series) on the
oracle's traces of base input A, the watt conversion, the all-reduce over two gloo ranks,
the C-ABI's struct and the `fleet` command's refusal without a GPU."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from series_util import A_N, A_STEPS, a_has_teeth, a_oracle
from tmhpvsim_amd import _lib, series

K = series.FRAC_BITS


def test_units_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert f"#define TMH_SERIES_FRAC_BITS {K}" in hdr
    assert K >= 12 and series.MAX_W >= 2.0 ** 14


def test_quantize_ties_exactness_nan():
    u = 2.0 ** -K
    # ties go to even
    np.testing.assert_array_equal(series.quantize(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.5]) * u), [0, 2, 2, 0, -2, 4])
    # every fp32 value below 2^14 W: x * 2^K is exact, so q is rint of the exact product
    g = np.random.default_rng(7)
    x = (g.random(20000) * 9000.0).astype(np.float32)
    x[:4] = [0.0, np.float32(8999.9995), np.float32(2.0 ** -20), np.float32(16383.999)]
    q = series.quantize(x)
    assert q.dtype == np.int64
    # (Python's round is half-to-even and float(v) * 2^K is exact)
    assert [int(v) for v in q[:200]] == [round(float(v) * 2 ** K) for v in x[:200]]
    assert (np.abs(q / 2.0 ** K - x.astype(np.float64)) <= 2.0 ** -(K + 1)).all()
    # fp32 input is taken in its own precision, not re-rounded
    np.testing.assert_array_equal(series.quantize(x), series.quantize(x.astype(np.float64)))
    np.testing.assert_array_equal(series.quantize(np.array([np.nan, 1.0, np.nan])), [0, 1 << K, 0])


def test_from_traces_on_input_a():
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    a_has_teeth(pv, cov, ref["status"])
    raw = series.from_traces(pv, meter, cov)
    assert raw.shape == (1, A_STEPS, 4) and raw.dtype == np.int64
    ok = ~np.isnan(pv)
    np.testing.assert_array_equal(ok, cov != 255)
    n_ok = ok.sum(axis=1)
    np.testing.assert_array_equal(raw[0, :, 2], n_ok)
    assert 900 < n_ok.min() <= n_ok.max() < A_N and n_ok.min() < n_ok.max()
    np.testing.assert_array_equal(raw[0, :, 3], (cov == 1).sum(axis=1))
    for col, tr in ((0, pv), (1, meter)):
        want = np.array([np.sum(r[o]) for r, o in zip(tr, ok)])          # fp64 sums of ~1,000 values
        slack = 1e-12 * np.abs(np.nan_to_num(tr)).sum(axis=1)            # their own rounding
        assert (np.abs(raw[0, :, col] / 2.0 ** K - want) <= n_ok * 2.0 ** -(K + 1) + slack).all()
    assert (raw[0, :, 0] == 0).any() and (raw[0, :, 0] > 0).any()        # night and daylight
    # partition-independent: 300 + 700 chains, added
    parts = series.from_traces(pv[:, :300], meter[:, :300], cov[:, :300]) + \
        series.from_traces(pv[:, 300:], meter[:, 300:], cov[:, 300:])
    np.testing.assert_array_equal(parts, raw)


def test_groups_of_512():
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    raw = series.from_traces(pv, meter, cov, group_chains=512)
    assert raw.shape == (2, A_STEPS, 4)
    np.testing.assert_array_equal(raw[0], series.from_traces(pv[:, :512], meter[:, :512], cov[:, :512])[0])
    np.testing.assert_array_equal(raw[1], series.from_traces(pv[:, 512:], meter[:, 512:], cov[:, 512:])[0])
    np.testing.assert_array_equal(raw.sum(axis=0), series.from_traces(pv, meter, cov)[0])
    assert raw[0, :, 2].max() <= 512 and raw[1, :, 2].max() <= 488
    # a series buffer with room for a third group: 512, 488 and 0 chains
    raw3 = series.from_traces(pv, meter, cov, group_chains=512, n_groups=3)
    assert raw3.shape == (3, A_STEPS, 4) and not raw3[2].any()
    np.testing.assert_array_equal(raw3[:2], raw)
    with pytest.raises(ValueError):
        series.from_traces(pv, meter, cov, group_chains=512, n_groups=1)
    # exactly 1,024 chains: two full groups, no third; 1,025: a third with one chain
    z = np.zeros((3, 1025))
    c = np.zeros((3, 1025), dtype=np.uint8)
    assert series.from_traces(z[:, :1024], z[:, :1024], c[:, :1024], 512).shape[0] == 2
    three = series.from_traces(z, z, c, 512)
    assert three.shape[0] == 3 and (three[2, :, 2] == 1).all()
    # no chains at all: one group of zeros
    assert not series.from_traces(z[:, :0], z[:, :0], c[:, :0], 512).any()
    with pytest.raises(ValueError):
        series.from_traces(z, z, c, 100)


def test_to_watts_bins():
    ref = a_oracle()
    raw = series.from_traces(ref["pv"], ref["meter"], ref["covered"])
    w1 = series.to_watts(raw)
    assert w1["pv"].shape == (1, A_STEPS)
    np.testing.assert_array_equal(w1["residual"], (raw[..., 1] - raw[..., 0]) / 2.0 ** K)
    nb = -(-A_STEPS // 60)
    assert A_STEPS % 60 == 3
    w = series.to_watts(raw, bin_s=60)
    m = series.to_watts(raw, bin_s=60, mean=True)
    for d in (w, m):
        assert all(v.shape == (1, nb) for v in d.values())
    for b in (0, 7, nb - 2, nb - 1):   # the last bin holds 3 seconds
        sl = raw[0, 60 * b:60 * (b + 1)].sum(axis=0)
        assert w["pv"][0, b] == sl[0] / 2.0 ** K and w["meter"][0, b] == sl[1] / 2.0 ** K
        assert w["n_ok"][0, b] == sl[2] and w["covered"][0, b] == sl[3] / sl[2]
        assert m["pv"][0, b] == sl[0] / (sl[2] * 2.0 ** K)
        assert m["residual"][0, b] == (sl[1] - sl[0]) / (sl[2] * 2.0 ** K)
    assert w["n_ok"][0, nb - 1] == raw[0, -3:, 2].sum()
    # a bin without an ok chain-second: NaN, not a division error
    e = np.zeros((1, 5, 4), dtype=np.int64)
    e[0, :2] = [[4096, 8192, 2, 1], [0, 4096, 2, 0]]
    out = series.to_watts(e, bin_s=2, mean=True)
    assert out["meter"][0, 0] == 12288 / (4 * 2.0 ** K) and out["pv"][0, 0] == 4096 / (4 * 2.0 ** K)
    assert np.isnan(out["pv"][0, 1:]).all() and np.isnan(out["covered"][0, 1:]).all()
    assert (out["n_ok"][0] == [4, 0, 0]).all()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _local_series(rank):
    g = np.random.default_rng(100 + rank)
    return g.integers(-(1 << 40), 1 << 40, size=(2, 37, 4), dtype=np.int64)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, series.all_reduce_series(torch.as_tensor(_local_series(rank))).numpy().copy()))
    finally:
        dist.destroy_process_group()


def test_all_reduce_series_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _local_series(0) + _local_series(1)
    for r in range(world):
        np.testing.assert_array_equal(res[r], want)
    one = series.all_reduce_series(_local_series(0))     # no process group: a copy
    np.testing.assert_array_equal(one.numpy(), _local_series(0))


def test_series_abi():
    L = _lib.load()
    assert C.sizeof(_lib.Series) == 8 + 8 + 4 * 4
    assert L.tmh_series_frac_bits() == K and L.tmh_series_max_w() == series.MAX_W
    s = _lib.Series(None, 0, 10, 0, 1, 0)
    assert L.tmh_set_series(None, C.byref(s)) == -1
    assert b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_series(None, None) == -1
    assert L.tmh_test_guard_records(None, None, 1, 1) == -1


def test_fleet_command_needs_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import main
    f = tmp_path / "fleet.csv"
    r = CliRunner().invoke(main, ["fleet", str(f), "--batch", "8", "--no-realtime", "--seconds", "60"])
    assert r.exit_code != 0 and "no GPU is visible" in r.output
    assert not f.exists()
    r = CliRunner().invoke(main, ["fleet", str(f), "--batch", "8"])      # realtime: refused as for pvsim
    assert r.exit_code != 0 and "--no-realtime" in r.output
