#!/usr/bin/env python
"""Cost of interval metering: TMH_K_EXPAND (tmh_profile_*: HIP events around the expansion
kernel) of the statistics-only expansion without and with intervals, same chains, same
window, same process, the two alternating.

    python scripts/intervals_cost.py [--chains 65536] [--steps 86400] [--interval 900] [--pairs 5]
                                     [--precision fp32] [--start "2019-09-05 00:00:00"] [--out FILE.json]

Without intervals the run launches the statistics-only instantiation (OUT_STATS), with
them the intervals instantiation (OUT_INTERVALS) with the same statistics beside it; the
script checks both variants, that the statistics of the two agree bit for bit and that the
table's ok seconds equal the histogram's count.  Prints one JSON line: the per-run
milliseconds, their medians and ranges, the ratio and the device's name.  Needs a GPU (no
fallback).  The script sets no time limit of its own: all runs share one process (same code
objects, same allocator), so the caller wraps it, e.g. `timeout -k 10 240 python
scripts/intervals_cost.py`; a run that hangs ends the measurement, nothing is retried."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=86400)
    ap.add_argument("--interval", type=int, default=900)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--start", default="2019-09-05 00:00:00")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import ModelParams
    if not torch.cuda.is_available():
        sys.exit("intervals_cost.py needs a GPU")

    def one(ivl):
        sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=ModelParams(), precision=a.precision,
                         device="cuda:0", horizon=a.steps)
        sim.enable_stats()
        raw = sim.enable_intervals(a.steps, a.interval) if ivl else None
        _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
        sim.run(a.steps, trace=(), window=a.steps)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
        want = (_lib.OUT_INTERVALS if ivl else _lib.OUT_STATS) | (_lib.OUT_FP64 if a.precision == "fp64" else 0)
        assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
        if ivl:
            assert int(raw[:, 2].sum()) == int(sim.hist.sum()) > 0
        return ms, sim.hist.clone(), sim.chain_acc.clone()

    one(False), one(True)   # warm-up: code objects, allocator
    t = {False: [], True: []}
    ref = None
    for _ in range(a.pairs):
        for s in (False, True):
            ms, hist, acc = one(s)
            t[s].append(ms)
            if ref is None:
                ref = (hist, acc)
            assert torch.equal(hist, ref[0]) and torch.equal(acc.view(torch.int64), ref[1].view(torch.int64))
    m0, m1 = statistics.median(t[False]), statistics.median(t[True])
    res = dict(device=torch.cuda.get_device_name(0), chains=a.chains, steps=a.steps, interval_s=a.interval,
               precision=a.precision, start=a.start, stats_only_ms=t[False], with_intervals_ms=t[True],
               stats_only_median_ms=m0, with_intervals_median_ms=m1,
               stats_only_range_ms=[min(t[False]), max(t[False])], with_intervals_range_ms=[min(t[True]), max(t[True])],
               ratio=m1 / m0, ns_per_chain_second=[1e6 * m0 / (a.chains * a.steps), 1e6 * m1 / (a.chains * a.steps)],
               build_stamp=_lib.loaded_stamp())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
