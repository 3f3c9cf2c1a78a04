#!/usr/bin/env python
"""Cost of an interval table: TMH_K_EXPAND (tmh_profile_*: HIP events around the expansion
kernel) of the statistics-only expansion and of the expansions with a table, same chains,
same window, same process, the runs alternating.

    python scripts/table_cost.py --kind intervals|registers|demand|storage|battery|battery_fleet|battery_sweep|dispatch|dispatch_sweep|schedule
                                 [--variants 5] [--rules 1] [--chains 65536] [--steps 86400]
                                 [--interval 900] [--rounds 5] [--precision fp32]
                                 [--start "2019-09-05 00:00:00"] [--out FILE.json]
                                 [--modules 1 --capacity-wh 5000 --charge-w 2500 --discharge-w 2500]
                                 [--charge-eff 0.95 --discharge-eff 0.95 --standby-w 2]
                                 [--charge-above-w 500 --discharge-above-w 200 --feed-in-limit-w 1000]

The runs of a kind, each with the same statistics beside its table:
  intervals: OUT_STATS and OUT_INTERVALS;
  registers: OUT_STATS, OUT_INTERVALS and OUT_REGISTERS -- the registers' first four columns
             are the intervals' table and import - export == meter - pv in every cell;
  demand:    OUT_STATS, OUT_REGISTERS and OUT_DEMAND -- the demand table's first six columns
             are the registers' table and every cell with an ok second has both keys (offset
             inside the interval, peak x n_ok >= the sum);
  storage:   OUT_STATS, OUT_REGISTERS and OUT_STORAGE, on an fp64 engine (the script sets the precision) --
             the storage table's first four columns are the registers' and [4] - [5] == [1] - [0] + [6] - [7]
             in every cell; its three launches (map pass, scan, replay) are timed separately as well
             (TMH_K_STORAGE_*), inside the TMH_K_EXPAND span.  --modules k scales the PV system (k modules) so
             that the battery of --capacity-wh / --charge-w / --discharge-w charges and discharges.
  battery:   OUT_STATS, OUT_STORAGE and OUT_BATTERY on an fp64 engine -- storage's setting with --charge-eff,
             --discharge-eff and --standby-w; the battery table's identities, a loss, and battery / storage for
             the whole expansion and for each of the three launches (the same TMH_K_STORAGE_* slots time both).
  battery_fleet: OUT_BATTERY and OUT_BATTERY_FLEET, battery's setting -- the battery kind alone and with its
             fleet series (BatchedSim.enable_battery_fleet, one group); the two tables are equal, the rows summed
             over each interval are the table summed over the chains; fleet / battery for the whole expansion and
             for each launch (the replay pass fills the rows), beside the spread of the kind's own rounds.
  battery_sweep: OUT_BATTERY and OUT_BATTERY_SWEEP, battery's setting, no statistics -- the unchanged battery kind
             (one battery of --capacity-wh per chain) and the sweep over --variants K capacities spread +-20 % around
             it, alternating; variant (K - 1) / 2 has the kind's own capacity and its table and soc are the kind's bit
             for bit, and columns 0-3 agree in every variant.  The kind's three launches are timed for both (the
             sweep's slots sum its groups' launches); the yardstick is K x the battery kind's median of the same run:
             ratio_sweep_k_battery = sweep / (K x battery) for the whole expansion and per launch, beside the spread
             of each run's own rounds.
  dispatch:  OUT_BATTERY and OUT_DISPATCH, battery's setting with statistics beside both -- the battery kind and battery
             dispatch with the same batteries plus --charge-above-w, --discharge-above-w and --feed-in-limit-w,
             alternating; the script checks that the thresholds and the limit bind (less is charged and discharged
             than under the battery kind, energy is curtailed, the peak fed in is the limit) and the dispatch
             table's identities.  The kind's three launches are timed for both; dispatch / battery for the whole
             expansion and per launch, with medians and ranges, beside the spread of the battery kind's own rounds.
  dispatch_sweep: OUT_DISPATCH and OUT_DISPATCH_SWEEP, dispatch's setting, no statistics -- the unchanged dispatch kind
             (one rule per chain: --charge-above-w, --discharge-above-w, --feed-in-limit-w) and the dispatch sweep over
             --variants K rule sets, the three quantities scaled by factors spread over [0.6, 1.4] around it,
             alternating; variant (K - 1) / 2 has the kind's own rule and its table and soc are the kind's bit for bit,
             columns 0-3 agree in every variant and every variant keeps the dispatch table's identities.  The kind's
             three launches are timed for both (the sweep's slots sum its groups' launches); the yardstick is K x the
             dispatch kind's median of the same run: ratio_sweep_k_dispatch = sweep / (K x dispatch) for the whole
             expansion and per launch, beside the spread of each run's own rounds.
  schedule:  OUT_DISPATCH and OUT_SCHEDULE, dispatch's setting with statistics beside both -- the unchanged dispatch kind
             (one rule per chain) and scheduled dispatch, alternating.  --rules 1: the schedule has that one rule, and
             the warm-up round's tables and soc are the dispatch kind's bit for bit.  --rules 4: four hourly rules (the
             rule of interval k is (k * interval // 3600) % 4) -- dispatch's own, one charging from the grid at a fifth of
             --charge-w, a hold, and dispatch's with the thresholds and the limit halved; the script checks the schedule
             table's identities, that the grid rule's intervals never discharge, the hold's neither charge nor
             discharge, and that the table differs from the dispatch kind's.  The kind's three launches are timed for
             both; schedule / dispatch for the whole expansion and per launch, with medians and ranges, beside the
             spread (max / min) of the dispatch kind's own rounds.
The script checks each run's variant, these identities (on the warm-up round's tables), that
the statistics of all runs agree bit for bit and that every table's ok seconds equal the
histogram's count.  One warm-up round, then --rounds timed ones.  Prints one JSON line: the
per-run milliseconds, their medians and ranges, the ratios between the runs and the device's
name.  Needs a GPU (no fallback).  The script sets no time limit of its own: all runs share
one process (same code objects, same allocator), so the caller wraps it, e.g. `timeout -k 10
300 python scripts/table_cost.py --kind demand`; a run that hangs ends the measurement,
nothing is retried."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# per kind: the runs as (label in the JSON keys, table enabled or None)
RUNS = {
    "intervals": (("stats_only", None), ("with_intervals", "intervals")),
    "registers": (("stats_only", None), ("intervals", "intervals"), ("registers", "registers")),
    "demand": (("stats_only", None), ("registers", "registers"), ("demand", "demand")),
    "storage": (("stats_only", None), ("registers", "registers"), ("storage", "storage")),
    "battery": (("stats_only", None), ("storage", "storage"), ("battery", "battery")),
    # (the table of both runs is the battery kind's; "battery_fleet" also enables the battery fleet series)
    "battery_fleet": (("battery", "battery"), ("battery_fleet", "battery")),
    "battery_sweep": (("battery", "battery"), ("battery_sweep", "battery_sweep")),   # (sweep_cost: a loop of its own)
    "dispatch": (("battery", "battery"), ("dispatch", "dispatch")),                  # (dispatch_cost: likewise)
    "dispatch_sweep": (("dispatch", "dispatch"), ("dispatch_sweep", "dispatch_sweep")),   # (dsweep_cost: likewise)
    "schedule": (("dispatch", "dispatch"), ("schedule", "schedule")),                     # (schedule_cost: likewise)
}


def check_tables(kind, tables, interval_s):
    """The kind's identities between the warm-up tables; the cells with feed-in (None: not counted)."""
    import torch
    if kind == "registers":
        rg, iv = tables["registers"], tables["intervals"]
        assert torch.equal(rg[:, :4], iv) and torch.equal(rg[:, 4] - rg[:, 5], rg[:, 1] - rg[:, 0])
        return int((rg[:, 5] > 0).sum())
    if kind == "demand":
        dm, rg = tables["demand"], tables["registers"]
        assert torch.equal(dm[:, :6], rg)
        for col, reg in ((6, 4), (7, 5)):
            key, n_ok = dm[:, col], dm[:, 2]
            assert torch.equal(key != 0, n_ok > 0)
            off = torch.where(key != 0, 0xFFFFFFFF - (key & 0xFFFFFFFF), torch.zeros_like(key))
            assert int(off.max()) < interval_s and bool(((key >> 32) * n_ok >= dm[:, reg]).all())
        return int((dm[:, 7] >> 32 > 0).sum())
    if kind == "storage":
        st, rg = tables["storage"], tables["registers"]
        assert torch.equal(st[:, :4], rg[:, :4]) and bool((st[:, 4:8] >= 0).all())
        assert torch.equal(st[:, 4] - st[:, 5], st[:, 1] - st[:, 0] + st[:, 6] - st[:, 7])
        assert torch.equal(st[:, 8] != 0, st[:, 2] > 0) and int((st[:, 8] >> 40).max()) <= interval_s
        return int((st[:, 5] > 0).sum())
    if kind == "battery":
        bt, st = tables["battery"], tables["storage"]
        assert torch.equal(bt[:, :4], st[:, :4]) and bool((bt[:, 4:8] >= 0).all()) and bool((bt[:, 9] >= 0).all())
        assert torch.equal(bt[:, 4] - bt[:, 5], bt[:, 1] - bt[:, 0] + bt[:, 6] - bt[:, 7])
        assert torch.equal(bt[:, 8] != 0, bt[:, 2] > 0) and int((bt[:, 8] >> 40).max()) <= interval_s
        assert int(bt[:, 9].sum()) > 0 and int(bt[:, 6].sum()) > 0 and int(bt[:, 7].sum()) > 0
        return int((bt[:, 5] > 0).sum())
    if kind == "battery_fleet":   # the same table with and without the fleet series; the rows against it, per interval
        bt, fb, fl = tables["battery"], tables["battery_fleet"], tables["fleet_rows"]
        assert torch.equal(bt, fb) and bool((fl[..., 4:] >= 0).all())
        per = fl[0].reshape(-1, interval_s, 8).sum(dim=1) if fl.shape[1] % interval_s == 0 else None
        if per is not None:
            for col, tcol in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (7, 6)):
                assert torch.equal(per[:, col], bt[:, tcol].sum(dim=1)), (col, tcol)
        assert int(fl[..., 6].sum()) > 0 and int(fl[..., 5].sum()) > 0
        return int((bt[:, 5] > 0).sum())
    return None


def sweep_cost(a, mp, lossy):
    """--kind battery_sweep: the battery kind and the sweep over a.variants capacities, alternating."""
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    K = a.variants
    caps = [a.capacity_wh * (0.8 + 0.4 * v / max(K - 1, 1)) for v in range(K)] if K > 1 else [a.capacity_wh]
    mid = (K - 1) // 2
    caps[mid] = a.capacity_wh
    soc0 = [c / 2 for c in caps]   # (half full, as the kind's: the variants differ from their first second)
    parts = (("map", _lib.K_STORAGE_MAP), ("scan", _lib.K_STORAGE_SCAN), ("replay", _lib.K_STORAGE_REPLAY))
    groups = None

    def one(label):
        nonlocal groups
        sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=mp, precision="fp64", device="cuda:0", horizon=a.steps)
        if label == "battery":
            raw = sim.enable_battery(a.steps, a.interval, **lossy)
        else:
            raw = sim.enable_battery_sweep(a.steps, a.interval, **{**lossy, "capacity_wh": caps, "soc0_wh": soc0})
        _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
        sim.run(a.steps, trace=(), window=a.steps)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
        want = (_lib.OUT_BATTERY if label == "battery" else _lib.OUT_BATTERY_SWEEP) | _lib.OUT_FP64
        assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
        pm = {}
        for name, kk in parts:
            pm[name], pn = _lib.profile_read(sim._eng, kk)
            if label == "battery":
                assert pn == 1
            else:
                groups = pn
        return ms, pm, raw, sim.soc.clone()

    def check(bt, sw):   # the warm-up round's tables: the middle variant is the kind's, columns 0-3 every variant's
        assert torch.equal(sw[2][mid], bt[2]) and torch.equal(sw[3][mid], bt[3])
        for v in range(K):
            t = sw[2][v]
            assert torch.equal(t[:, :4], bt[2][:, :4]) and bool((t[:, 4:8] >= 0).all()) and bool((t[:, 9] >= 0).all())
            assert torch.equal(t[:, 4] - t[:, 5], t[:, 1] - t[:, 0] + t[:, 6] - t[:, 7])
            assert v == mid or not torch.equal(t[:, 4:], bt[2][:, 4:])
        assert int(bt[2][:, 6].sum()) > 0 and int(bt[2][:, 7].sum()) > 0 and int(bt[2][:, 9].sum()) > 0

    check(one("battery"), one("battery_sweep"))   # warm-up: code objects, allocator
    labels = ("battery", "battery_sweep")
    t = {k: [] for k in labels}
    pt = {k: {name: [] for name, _ in parts} for k in labels}
    for _ in range(a.rounds):
        for label in labels:
            ms, pm, _raw, _soc = one(label)
            t[label].append(ms)
            for name in pm:
                pt[label][name].append(pm[name])
            del _raw, _soc
    med = {k: statistics.median(t[k]) for k in labels}
    pmed = {k: {name: statistics.median(v) for name, v in pt[k].items()} for k in labels}
    res = dict(device=torch.cuda.get_device_name(0), chains=a.chains, steps=a.steps, interval_s=a.interval, precision="fp64",
               start=a.start, rounds=a.rounds, modules=a.modules, battery=lossy, variants=K, capacities_wh=caps,
               launch_groups=groups,
               **{f"{k}_ms": t[k] for k in labels}, **{f"{k}_median_ms": med[k] for k in labels},
               **{f"{k}_{name}_ms": v for k in labels for name, v in pt[k].items()},
               **{f"{k}_{name}_median_ms": v for k in labels for name, v in pmed[k].items()},
               **{f"{k}_spread": max(t[k]) / min(t[k]) for k in labels},
               **{f"{k}_replay_spread": max(pt[k]["replay"]) / min(pt[k]["replay"]) for k in labels},
               yardstick_ms=K * med["battery"], sweep_ms_per_variant=med["battery_sweep"] / K,
               ratio_sweep_k_battery=med["battery_sweep"] / (K * med["battery"]),
               **{f"ratio_{name}_sweep_k_battery": pmed["battery_sweep"][name] / (K * pmed["battery"][name]) for name, _ in parts},
               build_stamp=_lib.loaded_stamp())
    return res


def dispatch_cost(a, mp, lossy):
    """--kind dispatch: the battery kind and battery dispatch over the same batteries, alternating."""
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    rule = dict(charge_above_w=a.charge_above_w, discharge_above_w=a.discharge_above_w, feed_in_limit_w=a.feed_in_limit_w)
    parts = (("map", _lib.K_STORAGE_MAP), ("scan", _lib.K_STORAGE_SCAN), ("replay", _lib.K_STORAGE_REPLAY))
    labels = ("battery", "dispatch")

    def one(label):
        sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=mp, precision="fp64", device="cuda:0", horizon=a.steps)
        sim.enable_stats()
        raw = sim.enable_battery(a.steps, a.interval, **lossy) if label == "battery" else \
            sim.enable_dispatch(a.steps, a.interval, **lossy, **rule)
        _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
        sim.run(a.steps, trace=(), window=a.steps)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
        want = (_lib.OUT_BATTERY if label == "battery" else _lib.OUT_DISPATCH) | _lib.OUT_FP64
        assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
        pm = {}
        for name, kk in parts:
            pm[name], pn = _lib.profile_read(sim._eng, kk)
            assert pn == 1
        assert int(raw[:, 2].sum()) == int(sim.hist.sum()) > 0
        return ms, pm, raw, sim.hist.clone()

    def check(bt, dp):   # the warm-up round's tables: the same seconds, the rule binds, the dispatch table's identities
        b, d = bt[2], dp[2]
        assert torch.equal(d[:, :4], b[:, :4]) and torch.equal(bt[3], dp[3])
        assert bool((d[:, 4:8] >= 0).all()) and bool((d[:, 9:11] >= 0).all())
        assert torch.equal(d[:, 4] - d[:, 5], d[:, 1] - d[:, 0] + d[:, 6] - d[:, 7] + d[:, 10])
        assert torch.equal(d[:, 11] != 0, d[:, 2] > 0) and torch.equal(d[:, 12] != 0, d[:, 2] > 0)
        lim = int(round(a.feed_in_limit_w * 4096))
        assert int((d[:, 12] >> 32).max()) == lim and int(d[:, 10].sum()) > 0                    # the limit binds
        assert 0 < int(d[:, 6].sum()) < int(b[:, 6].sum()) and 0 < int(d[:, 7].sum()) < int(b[:, 7].sum())   # the thresholds bind
        return dict(curtailed_share=int(d[:, 10].sum()) / int(d[:, 0].sum()), curtail_cells=int((d[:, 10] > 0).sum()),
                    charge_dispatch_over_battery=int(d[:, 6].sum()) / int(b[:, 6].sum()),
                    discharge_dispatch_over_battery=int(d[:, 7].sum()) / int(b[:, 7].sum()))

    binds = check(one("battery"), one("dispatch"))   # warm-up: code objects, allocator
    t = {k: [] for k in labels}
    pt = {k: {name: [] for name, _ in parts} for k in labels}
    for _ in range(a.rounds):
        for label in labels:
            ms, pm, _raw, _hist = one(label)
            t[label].append(ms)
            for name in pm:
                pt[label][name].append(pm[name])
            del _raw, _hist
    med = {k: statistics.median(t[k]) for k in labels}
    pmed = {k: {name: statistics.median(v) for name, v in pt[k].items()} for k in labels}
    return dict(device=torch.cuda.get_device_name(0), chains=a.chains, steps=a.steps, interval_s=a.interval, precision="fp64",
                start=a.start, rounds=a.rounds, modules=a.modules, battery=lossy, rule=rule, **binds,
                **{f"{k}_ms": t[k] for k in labels}, **{f"{k}_median_ms": med[k] for k in labels},
                **{f"{k}_range_ms": [min(t[k]), max(t[k])] for k in labels},
                **{f"{k}_{name}_ms": v for k in labels for name, v in pt[k].items()},
                **{f"{k}_{name}_median_ms": v for k in labels for name, v in pmed[k].items()},
                **{f"{k}_{name}_range_ms": [min(v), max(v)] for k in labels for name, v in pt[k].items()},
                ratio_dispatch_battery=med["dispatch"] / med["battery"],
                **{f"ratio_{name}_dispatch_battery": pmed["dispatch"][name] / pmed["battery"][name] for name, _ in parts},
                battery_spread=max(t["battery"]) / min(t["battery"]),
                **{f"battery_{name}_spread": max(v) / min(v) for name, v in pt["battery"].items()},
                build_stamp=_lib.loaded_stamp())


def dsweep_cost(a, mp, lossy):
    """--kind dispatch_sweep: the dispatch kind and the dispatch sweep over a.variants rule sets, alternating."""
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    K = a.variants
    mid = (K - 1) // 2
    fac = [0.6 + 0.8 * v / (K - 1) for v in range(K)] if K > 1 else [1.0]
    fac[mid] = 1.0
    rule = dict(charge_above_w=a.charge_above_w, discharge_above_w=a.discharge_above_w, feed_in_limit_w=a.feed_in_limit_w)
    rules = {k: [w * f for f in fac] for k, w in rule.items()}
    parts = (("map", _lib.K_STORAGE_MAP), ("scan", _lib.K_STORAGE_SCAN), ("replay", _lib.K_STORAGE_REPLAY))
    labels = ("dispatch", "dispatch_sweep")
    groups = None

    def one(label):
        nonlocal groups
        sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=mp, precision="fp64", device="cuda:0", horizon=a.steps)
        if label == "dispatch":
            raw = sim.enable_dispatch(a.steps, a.interval, **lossy, **rule)
        else:
            raw = sim.enable_dispatch_sweep(a.steps, a.interval, n_variants=K, **lossy, **rules)
        _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
        sim.run(a.steps, trace=(), window=a.steps)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
        want = (_lib.OUT_DISPATCH if label == "dispatch" else _lib.OUT_DISPATCH_SWEEP) | _lib.OUT_FP64
        assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
        pm = {}
        for name, kk in parts:
            pm[name], pn = _lib.profile_read(sim._eng, kk)
            if label == "dispatch":
                assert pn == 1
            else:
                groups = pn
        return ms, pm, raw, sim.soc.clone()

    def check(dp, sw):   # the warm-up round's tables: the middle variant is the kind's, columns 0-3 every variant's
        assert torch.equal(sw[2][mid], dp[2]) and torch.equal(sw[3][mid], dp[3])
        for v in range(K):
            t = sw[2][v]
            assert torch.equal(t[:, :4], dp[2][:, :4]) and bool((t[:, 4:8] >= 0).all()) and bool((t[:, 9:11] >= 0).all())
            assert torch.equal(t[:, 4] - t[:, 5], t[:, 1] - t[:, 0] + t[:, 6] - t[:, 7] + t[:, 10])
            assert torch.equal(t[:, 11] != 0, t[:, 2] > 0) and torch.equal(t[:, 12] != 0, t[:, 2] > 0)
            assert int((t[:, 12] >> 32).max()) == int(round(rules["feed_in_limit_w"][v] * 4096)) and int(t[:, 10].sum()) > 0
            assert v == mid or not torch.equal(t[:, 4:], dp[2][:, 4:])
        d = dp[2]
        assert int(d[:, 6].sum()) > 0 and int(d[:, 7].sum()) > 0 and int(d[:, 9].sum()) > 0
        return [int(sw[2][v][:, 10].sum()) / int(d[:, 0].sum()) for v in range(K)]

    shares = check(one("dispatch"), one("dispatch_sweep"))   # warm-up: code objects, allocator
    t = {k: [] for k in labels}
    pt = {k: {name: [] for name, _ in parts} for k in labels}
    for _ in range(a.rounds):
        for label in labels:
            ms, pm, _raw, _soc = one(label)
            t[label].append(ms)
            for name in pm:
                pt[label][name].append(pm[name])
            del _raw, _soc
    med = {k: statistics.median(t[k]) for k in labels}
    pmed = {k: {name: statistics.median(v) for name, v in pt[k].items()} for k in labels}
    return dict(device=torch.cuda.get_device_name(0), chains=a.chains, steps=a.steps, interval_s=a.interval, precision="fp64",
                start=a.start, rounds=a.rounds, modules=a.modules, battery=lossy, variants=K, rules=rules,
                curtailed_shares=shares, launch_groups=groups,
                **{f"{k}_ms": t[k] for k in labels}, **{f"{k}_median_ms": med[k] for k in labels},
                **{f"{k}_range_ms": [min(t[k]), max(t[k])] for k in labels},
                **{f"{k}_{name}_ms": v for k in labels for name, v in pt[k].items()},
                **{f"{k}_{name}_median_ms": v for k in labels for name, v in pmed[k].items()},
                **{f"{k}_spread": max(t[k]) / min(t[k]) for k in labels},
                **{f"{k}_replay_spread": max(pt[k]["replay"]) / min(pt[k]["replay"]) for k in labels},
                yardstick_ms=K * med["dispatch"], sweep_ms_per_variant=med["dispatch_sweep"] / K,
                ratio_sweep_k_dispatch=med["dispatch_sweep"] / (K * med["dispatch"]),
                **{f"ratio_{name}_sweep_k_dispatch": pmed["dispatch_sweep"][name] / (K * pmed["dispatch"][name]) for name, _ in parts},
                build_stamp=_lib.loaded_stamp())


def schedule_cost(a, mp, lossy):
    """--kind schedule: the dispatch kind and scheduled dispatch (a.rules rule sets) over the same batteries, alternating."""
    import numpy as np
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    rule = dict(charge_above_w=a.charge_above_w, discharge_above_w=a.discharge_above_w, feed_in_limit_w=a.feed_in_limit_w)
    n_iv = -(-a.steps // a.interval)
    if a.rules == 1:
        rules, roi = [dict(rule, grid_charge_w=0.0)], np.zeros(n_iv, dtype=np.uint8)
    elif a.rules == 4:
        rules = [dict(rule, grid_charge_w=0.0),
                 dict(rule, grid_charge_w=a.charge_w / 5),
                 dict(charge_above_w=32768.0, discharge_above_w=32768.0, feed_in_limit_w=a.feed_in_limit_w, grid_charge_w=0.0),
                 dict(charge_above_w=a.charge_above_w / 2, discharge_above_w=a.discharge_above_w / 2,
                      feed_in_limit_w=a.feed_in_limit_w / 2, grid_charge_w=0.0)]
        roi = ((np.arange(n_iv) * a.interval // 3600) % 4).astype(np.uint8)
    else:
        sys.exit("--kind schedule: --rules 1 or 4")
    parts = (("map", _lib.K_STORAGE_MAP), ("scan", _lib.K_STORAGE_SCAN), ("replay", _lib.K_STORAGE_REPLAY))
    labels = ("dispatch", "schedule")

    def one(label):
        sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=mp, precision="fp64", device="cuda:0", horizon=a.steps)
        sim.enable_stats()
        raw = sim.enable_dispatch(a.steps, a.interval, **lossy, **rule) if label == "dispatch" else \
            sim.enable_schedule(a.steps, a.interval, **lossy, rules=rules, rule_of_interval=roi)
        _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
        sim.run(a.steps, trace=(), window=a.steps)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
        want = (_lib.OUT_DISPATCH if label == "dispatch" else _lib.OUT_SCHEDULE) | _lib.OUT_FP64
        assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
        pm = {}
        for name, kk in parts:
            pm[name], pn = _lib.profile_read(sim._eng, kk)
            assert pn == 1
        assert int(raw[:, 2].sum()) == int(sim.hist.sum()) > 0
        return ms, pm, raw, sim.hist.clone(), sim.soc.clone()

    def check(dp, sc):   # the warm-up round's tables
        d, s = dp[2], sc[2]
        assert torch.equal(s[:, :4], d[:, :4]) and torch.equal(dp[3], sc[3])
        assert bool((s[:, 4:8] >= 0).all()) and bool((s[:, 9:11] >= 0).all())
        assert torch.equal(s[:, 4] - s[:, 5], s[:, 1] - s[:, 0] + s[:, 6] - s[:, 7] + s[:, 10])
        assert torch.equal(s[:, 11] != 0, s[:, 2] > 0) and torch.equal(s[:, 12] != 0, s[:, 2] > 0)
        assert int(d[:, 6].sum()) > 0 and int(d[:, 7].sum()) > 0 and int(d[:, 10].sum()) > 0
        if a.rules == 1:   # the same rule: the dispatch kind's bits
            assert torch.equal(s, d) and torch.equal(dp[4], sc[4])
            return dict(tables_equal=True)
        r = torch.from_numpy(roi.astype(np.int64)).to(s.device)
        lim = torch.tensor([int(round(x["feed_in_limit_w"] * 4096)) for x in rules], device=s.device)[r]
        assert bool(((s[:, 12] >> 32) <= lim[:, None]).all())
        assert not bool(s[r == 1, 7].any()) and int(s[r == 1, 6].sum()) > 0          # the grid rule never discharges
        assert not bool(s[r == 2, 6].any()) and not bool(s[r == 2, 7].any())         # hold
        assert not torch.equal(s[:, 4:], d[:, 4:])
        return dict(tables_equal=False, differing_cells_import=int((s[:, 4] != d[:, 4]).sum()),
                    import_schedule_over_dispatch=int(s[:, 4].sum()) / int(d[:, 4].sum()),
                    charge_schedule_over_dispatch=int(s[:, 6].sum()) / int(d[:, 6].sum()))

    found = check(one("dispatch"), one("schedule"))   # warm-up: code objects, allocator
    t = {k: [] for k in labels}
    pt = {k: {name: [] for name, _ in parts} for k in labels}
    for _ in range(a.rounds):
        for label in labels:
            ms, pm, _raw, _hist, _soc = one(label)
            t[label].append(ms)
            for name in pm:
                pt[label][name].append(pm[name])
            del _raw, _hist, _soc
    med = {k: statistics.median(t[k]) for k in labels}
    pmed = {k: {name: statistics.median(v) for name, v in pt[k].items()} for k in labels}
    return dict(device=torch.cuda.get_device_name(0), chains=a.chains, steps=a.steps, interval_s=a.interval, precision="fp64",
                start=a.start, rounds=a.rounds, modules=a.modules, battery=lossy, n_rules=a.rules, rules=rules,
                rule_of_interval=roi.tolist(), **found,
                **{f"{k}_ms": t[k] for k in labels}, **{f"{k}_median_ms": med[k] for k in labels},
                **{f"{k}_range_ms": [min(t[k]), max(t[k])] for k in labels},
                **{f"{k}_{name}_ms": v for k in labels for name, v in pt[k].items()},
                **{f"{k}_{name}_median_ms": v for k in labels for name, v in pmed[k].items()},
                **{f"{k}_{name}_range_ms": [min(v), max(v)] for k in labels for name, v in pt[k].items()},
                ratio_schedule_dispatch=med["schedule"] / med["dispatch"],
                **{f"ratio_{name}_schedule_dispatch": pmed["schedule"][name] / pmed["dispatch"][name] for name, _ in parts},
                dispatch_spread=max(t["dispatch"]) / min(t["dispatch"]),
                **{f"dispatch_{name}_spread": max(v) / min(v) for name, v in pt["dispatch"].items()},
                build_stamp=_lib.loaded_stamp())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=tuple(RUNS), required=True)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=86400)
    ap.add_argument("--interval", type=int, default=900)
    ap.add_argument("--rounds", "--pairs", type=int, default=5)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--start", default="2019-09-05 00:00:00")
    ap.add_argument("--out", default=None)
    ap.add_argument("--modules", type=int, default=1, help="PV modules per chain (the inverter scaled alike)")
    ap.add_argument("--capacity-wh", type=float, default=5000.0)
    ap.add_argument("--charge-w", type=float, default=2500.0)
    ap.add_argument("--discharge-w", type=float, default=2500.0)
    ap.add_argument("--charge-eff", type=float, default=0.95)
    ap.add_argument("--discharge-eff", type=float, default=0.95)
    ap.add_argument("--standby-w", type=float, default=2.0)
    ap.add_argument("--variants", type=int, default=5, help="--kind battery_sweep, dispatch_sweep: the variants per chain")
    ap.add_argument("--rules", type=int, default=1, help="--kind schedule: 1 (the dispatch kind's rule) or 4 hourly rules")
    ap.add_argument("--charge-above-w", type=float, default=500.0, help="--kind dispatch: the charge threshold")
    ap.add_argument("--discharge-above-w", type=float, default=200.0, help="--kind dispatch: the discharge threshold")
    ap.add_argument("--feed-in-limit-w", type=float, default=1000.0, help="--kind dispatch: the feed-in limit")
    a = ap.parse_args()
    if a.kind in ("storage", "battery", "battery_fleet", "battery_sweep", "dispatch", "dispatch_sweep", "schedule"):
        a.precision = "fp64"   # (the kind's engines)
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import ModelParams
    if not torch.cuda.is_available():
        sys.exit("table_cost.py needs a GPU")
    out_of = {None: _lib.OUT_STATS, "intervals": _lib.OUT_INTERVALS, "registers": _lib.OUT_REGISTERS,
              "demand": _lib.OUT_DEMAND, "storage": _lib.OUT_STORAGE, "battery": _lib.OUT_BATTERY}
    parts = (("map", _lib.K_STORAGE_MAP), ("scan", _lib.K_STORAGE_SCAN), ("replay", _lib.K_STORAGE_REPLAY))
    part_ms = {name: [] for name, _ in parts}           # the kind's own launches
    below_ms = {name: [] for name, _ in parts}          # --kind battery: storage's, the run below it
    mp = ModelParams()
    if a.modules != 1:   # k modules on a k-fold inverter
        import dataclasses
        mod, inv = dict(mp.module), dict(mp.inverter)
        mod["Impo"] *= a.modules
        for key in ("Paco", "Pdco", "Pso", "Pnt"):
            inv[key] *= a.modules
        inv["C0"] /= a.modules
        mp = dataclasses.replace(mp, module=mod, inverter=inv)
    battery = dict(capacity_wh=a.capacity_wh, charge_w=a.charge_w, discharge_w=a.discharge_w, soc0_wh=a.capacity_wh / 2)
    lossy = dict(battery, charge_eff=a.charge_eff, discharge_eff=a.discharge_eff, standby_w=a.standby_w)
    enable_kw = {"storage": battery, "battery": lossy}
    if a.kind in ("battery_sweep", "dispatch", "dispatch_sweep", "schedule"):
        cost = {"battery_sweep": sweep_cost, "dispatch": dispatch_cost, "dispatch_sweep": dsweep_cost,
                "schedule": schedule_cost}[a.kind]
        line = json.dumps(cost(a, mp, lossy))
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
    runs = RUNS[a.kind]
    labels = [label for label, _ in runs]

    fleet_rows = {}

    def one(table, label=None):
        fleet = label == "battery_fleet"
        sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=mp, precision=a.precision,
                         device="cuda:0", horizon=a.steps)
        sim.enable_stats()
        raw = getattr(sim, "enable_" + table)(a.steps, a.interval, **enable_kw.get(table, {})) if table else None
        if fleet:
            fleet_rows["fleet_rows"] = sim.enable_battery_fleet(a.steps)
        _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
        sim.run(a.steps, trace=(), window=a.steps)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
        want = (_lib.OUT_BATTERY_FLEET if fleet else out_of[table]) | (_lib.OUT_FP64 if a.precision == "fp64" else 0)
        assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
        if table in ("storage", "battery"):   # its three launches, once each, inside the span read above
            for name, kk in parts:
                pms, pn = _lib.profile_read(sim._eng, kk)
                assert pn == 1
                (part_ms if (label or table) == a.kind else below_ms)[name].append(pms)
        if raw is not None:
            assert int(raw[:, 2].sum()) == int(sim.hist.sum()) > 0
        return ms, sim.hist.clone(), sim.chain_acc.clone(), raw

    by_label = a.kind == "battery_fleet"   # (both of its runs fill the battery kind's table)
    tables = {(label if by_label else table): one(table, label)[3] for label, table in runs}   # warm-up: code objects, allocator
    export_cells = check_tables(a.kind, {**tables, **fleet_rows}, a.interval)
    fleet_rows.clear()
    del tables
    for v in list(part_ms.values()) + list(below_ms.values()):
        v.clear()   # (the warm-up round's)
    t = {label: [] for label in labels}
    ref = None
    for _ in range(a.rounds):
        for label, table in runs:
            ms, hist, acc, _raw = one(table, label)
            t[label].append(ms)
            if ref is None:
                ref = (hist, acc)
            assert torch.equal(hist, ref[0]) and torch.equal(acc.view(torch.int64), ref[1].view(torch.int64))
    med = {label: statistics.median(t[label]) for label in labels}
    ns = {label: 1e6 * med[label] / (a.chains * a.steps) for label in labels}
    res = dict(device=torch.cuda.get_device_name(0), chains=a.chains, steps=a.steps, interval_s=a.interval,
               precision=a.precision, start=a.start,
               **{f"{k}_ms": t[k] for k in labels}, **{f"{k}_median_ms": med[k] for k in labels},
               **{f"{k}_range_ms": [min(t[k]), max(t[k])] for k in labels})
    if a.kind == "battery_fleet":   # the battery kind with its fleet series over the kind alone: the whole expansion
        pmed = {name: statistics.median(v) for name, v in part_ms.items()}      # and each launch (the replay pass fills
        bmed = {name: statistics.median(v) for name, v in below_ms.items()}     # the rows), beside the spread of the
        res.update(rounds=a.rounds, export_cells=export_cells, modules=a.modules, battery=lossy, ns_per_chain_second=ns,
                   **{f"battery_fleet_{k}_ms": v for k, v in part_ms.items()}, **{f"battery_{k}_ms": v for k, v in below_ms.items()},
                   **{f"battery_fleet_{k}_median_ms": v for k, v in pmed.items()},
                   **{f"battery_{k}_median_ms": v for k, v in bmed.items()},
                   **{f"ratio_{k}_fleet_battery": pmed[k] / bmed[k] for k in pmed},
                   ratio_fleet_battery=med["battery_fleet"] / med["battery"],
                   battery_spread=max(t["battery"]) / min(t["battery"]),      # kind's own rounds
                   battery_replay_spread=max(below_ms["replay"]) / min(below_ms["replay"]))
    elif a.kind == "intervals":
        res.update(ratio=med["with_intervals"] / med["stats_only"], ns_per_chain_second=[ns[k] for k in labels])
    else:   # the kind over the statistics, the kind over the table below it, that table over the statistics
        below = labels[1]
        res.update(rounds=a.rounds, export_cells=export_cells,
                   **{f"ratio_{a.kind}_stats": med[a.kind] / med["stats_only"],
                      f"ratio_{a.kind}_{below}": med[a.kind] / med[below],
                      f"ratio_{below}_stats": med[below] / med["stats_only"]},
                   ns_per_chain_second=ns)
    if a.kind == "storage":
        pmed = {name: statistics.median(v) for name, v in part_ms.items()}
        res.update(modules=a.modules, battery=battery, **{f"storage_{k}_ms": v for k, v in part_ms.items()},
                   **{f"storage_{k}_median_ms": v for k, v in pmed.items()},
                   scan_share=pmed["scan"] / med["storage"], ratio_replay_registers=pmed["replay"] / med["registers"],
                   ratio_map_registers=pmed["map"] / med["registers"], scan_over_replay=pmed["scan"] / pmed["replay"])
    if a.kind == "battery":   # battery / storage: the whole expansion and each launch, beside the spread of storage's own rounds
        pmed = {name: statistics.median(v) for name, v in part_ms.items()}
        smed = {name: statistics.median(v) for name, v in below_ms.items()}
        res.update(modules=a.modules, battery=lossy,
                   **{f"battery_{k}_ms": v for k, v in part_ms.items()}, **{f"storage_{k}_ms": v for k, v in below_ms.items()},
                   **{f"battery_{k}_median_ms": v for k, v in pmed.items()},
                   **{f"storage_{k}_median_ms": v for k, v in smed.items()},
                   **{f"ratio_{k}_battery_storage": pmed[k] / smed[k] for k in pmed},
                   storage_spread=max(t["storage"]) / min(t["storage"]))
    res["build_stamp"] = _lib.loaded_stamp()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
