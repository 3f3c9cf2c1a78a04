#!/usr/bin/env python
"""Cost of the demand registers: TMH_K_EXPAND (tmh_profile_*: HIP events around the expansion
kernel) of the statistics-only expansion, of the import / export registers and of the demand
registers, same chains, same window, same process, the three alternating.

    python scripts/demand_cost.py [--chains 65536] [--steps 86400] [--interval 900] [--rounds 5]
                                  [--precision fp32] [--start "2019-09-05 00:00:00"] [--out FILE.json]

The three runs launch the OUT_STATS, OUT_REGISTERS and OUT_DEMAND instantiations with the
same statistics beside them; the script checks the variants, that the statistics of all runs
agree bit for bit, that the demand table's first six columns are the registers' table, that
every cell with an ok second has both keys (offset inside the interval, peak x n_ok >= the
sum) and that the table's ok seconds equal the histogram's count.  One warm-up round, then
--rounds timed ones.  Prints one JSON line: the per-run milliseconds, their min / median /
max, the ratios demand / statistics and demand / registers and the device's name.  Needs a
GPU (no fallback).  The script sets no time limit of its own: all runs share one process
(same code objects, same allocator), so the caller wraps it, e.g. `timeout -k 10 300 python
scripts/demand_cost.py`; a run that hangs ends the measurement, nothing is retried."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = ("stats_only", "registers", "demand")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=86400)
    ap.add_argument("--interval", type=int, default=900)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--start", default="2019-09-05 00:00:00")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import ModelParams
    if not torch.cuda.is_available():
        sys.exit("demand_cost.py needs a GPU")
    out_of = dict(stats_only=_lib.OUT_STATS, registers=_lib.OUT_REGISTERS, demand=_lib.OUT_DEMAND)

    def one(kind):
        sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=ModelParams(), precision=a.precision,
                         device="cuda:0", horizon=a.steps)
        sim.enable_stats()
        raw = None
        if kind == "registers":
            raw = sim.enable_registers(a.steps, a.interval)
        elif kind == "demand":
            raw = sim.enable_demand(a.steps, a.interval)
        _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
        sim.run(a.steps, trace=(), window=a.steps)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
        want = out_of[kind] | (_lib.OUT_FP64 if a.precision == "fp64" else 0)
        assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
        if raw is not None:
            assert int(raw[:, 2].sum()) == int(sim.hist.sum()) > 0
        return ms, sim.hist.clone(), sim.chain_acc.clone(), raw

    tables = {k: one(k)[3] for k in KINDS}   # warm-up: code objects, allocator
    dm, rg = tables["demand"], tables["registers"]
    assert torch.equal(dm[:, :6], rg)
    for col, reg in ((6, 4), (7, 5)):
        key, n_ok = dm[:, col], dm[:, 2]
        assert torch.equal(key != 0, n_ok > 0)
        off = torch.where(key != 0, 0xFFFFFFFF - (key & 0xFFFFFFFF), torch.zeros_like(key))
        assert int(off.max()) < a.interval and bool(((key >> 32) * n_ok >= dm[:, reg]).all())
    export_cells = int((dm[:, 7] >> 32 > 0).sum())
    del tables, dm, rg
    t = {k: [] for k in KINDS}
    ref = None
    for _ in range(a.rounds):
        for k in KINDS:
            ms, hist, acc, _raw = one(k)
            t[k].append(ms)
            if ref is None:
                ref = (hist, acc)
            assert torch.equal(hist, ref[0]) and torch.equal(acc.view(torch.int64), ref[1].view(torch.int64))
    med = {k: statistics.median(t[k]) for k in KINDS}
    res = dict(device=torch.cuda.get_device_name(0), chains=a.chains, steps=a.steps, interval_s=a.interval,
               precision=a.precision, start=a.start, rounds=a.rounds, export_cells=export_cells,
               **{f"{k}_ms": t[k] for k in KINDS}, **{f"{k}_median_ms": med[k] for k in KINDS},
               **{f"{k}_range_ms": [min(t[k]), max(t[k])] for k in KINDS},
               ratio_demand_stats=med["demand"] / med["stats_only"],
               ratio_demand_registers=med["demand"] / med["registers"],
               ratio_registers_stats=med["registers"] / med["stats_only"],
               ns_per_chain_second={k: 1e6 * med[k] / (a.chains * a.steps) for k in KINDS},
               build_stamp=_lib.loaded_stamp())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
