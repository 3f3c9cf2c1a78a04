#!/usr/bin/env python
"""Cost of an interval table: TMH_K_EXPAND (tmh_profile_*: HIP events around the expansion
kernel) of the statistics-only expansion and of the expansions with a table, same chains,
same window, same process, the runs alternating.

    python scripts/table_cost.py --kind intervals|registers|demand|storage|battery|battery_fleet|battery_sweep|dispatch|dispatch_sweep|schedule
                                        |dispatch_fleet|schedule_fleet|schedule_sweep
                                 [--variants 5] [--rules 1] [--chains 65536] [--steps 86400]
                                 [--interval 900] [--rounds 5] [--precision fp32]
                                 [--start "2019-09-05 00:00:00"] [--out FILE.json]
                                 [--modules 1 --capacity-wh 5000 --charge-w 2500 --discharge-w 2500]
                                 [--charge-eff 0.95 --discharge-eff 0.95 --standby-w 2]
                                 [--charge-above-w 500 --discharge-above-w 200 --feed-in-limit-w 1000]

The runs of a kind:
  intervals: OUT_STATS and OUT_INTERVALS;
  registers: OUT_STATS, OUT_INTERVALS and OUT_REGISTERS -- the registers' first four columns
             are the intervals' table and import - export == meter - pv in every cell;
  demand:    OUT_STATS, OUT_REGISTERS and OUT_DEMAND -- the demand table's first six columns
             are the registers' table and every cell with an ok second has both keys (offset
             inside the interval, peak x n_ok >= the sum);
  storage:   OUT_STATS, OUT_REGISTERS and OUT_STORAGE, on an fp64 engine (the script sets the precision, for this
             kind and all below) -- the storage table's first four columns are the registers' and
             [4] - [5] == [1] - [0] + [6] - [7] in every cell.  --modules k scales the PV system (k modules) so
             that the battery of --capacity-wh / --charge-w / --discharge-w charges and discharges.
  battery:   OUT_STATS, OUT_STORAGE and OUT_BATTERY -- storage's setting with --charge-eff, --discharge-eff and
             --standby-w; the battery table's identities and a loss.
  battery_fleet: OUT_BATTERY and OUT_BATTERY_FLEET, battery's setting -- the battery kind alone and with its
             fleet series (BatchedSim.enable_battery_fleet, one group); the two tables are equal, the rows summed
             over each interval are the table summed over the chains (the replay pass fills the rows).
  battery_sweep: OUT_BATTERY and OUT_BATTERY_SWEEP, battery's setting, no statistics -- the unchanged battery kind
             (one battery of --capacity-wh per chain) and the sweep over --variants K capacities spread +-20 % around
             it; variant (K - 1) / 2 has the kind's own capacity and its table and soc are the kind's bit for bit, and
             columns 0-3 agree in every variant.  The yardstick is K x the battery kind's median of the same run:
             ratio_sweep_k_battery = sweep / (K x battery) for the whole expansion and per launch (the sweep's slots
             sum its groups' launches: launch_groups).
  dispatch:  OUT_BATTERY and OUT_DISPATCH, battery's setting -- the battery kind and battery dispatch with the same
             batteries plus --charge-above-w, --discharge-above-w and --feed-in-limit-w; the script checks that the
             thresholds and the limit bind (less is charged and discharged than under the battery kind, energy is
             curtailed, the peak fed in is the limit) and the dispatch table's identities.
  dispatch_sweep: OUT_DISPATCH and OUT_DISPATCH_SWEEP, dispatch's setting, no statistics -- the unchanged dispatch kind
             (one rule per chain) and the dispatch sweep over --variants K rule sets, the three quantities scaled by
             factors spread over [0.6, 1.4] around it; the battery sweep's checks, and every variant keeps the dispatch
             table's identities.  The yardstick is K x the dispatch kind's median: ratio_sweep_k_dispatch likewise.
  schedule:  OUT_DISPATCH and OUT_SCHEDULE, dispatch's setting -- the unchanged dispatch kind and scheduled dispatch.
             --rules 1: the schedule has that one rule, and the warm-up round's tables and soc are the dispatch kind's
             bit for bit.  --rules 4: four hourly rules (the rule of interval k is (k * interval // 3600) % 4) --
             dispatch's own, one charging from the grid at a fifth of --charge-w, a hold, and dispatch's with the
             thresholds and the limit halved; the script checks the schedule table's identities, that the grid rule's
             intervals never discharge, the hold's neither charge nor discharge, and that the table differs from the
             dispatch kind's.
  dispatch_fleet: OUT_DISPATCH and OUT_DISPATCH_FLEET, dispatch's setting -- battery dispatch alone and with the
             dispatch fleet series (BatchedSim.enable_dispatch_fleet, one group); the two tables and soc are equal, the
             rows summed over each interval are the table summed over the chains (columns 0-5, 7 and 8 against 0-5, 6
             and 10), and the fleet curtails.
  schedule_fleet: OUT_SCHEDULE and OUT_SCHEDULE_FLEET, schedule's setting (--rules 1|4) -- the schedule alone and with
             the dispatch fleet series; dispatch_fleet's checks.
  schedule_sweep: OUT_SCHEDULE and OUT_SCHEDULE_SWEEP, schedule's setting with --rules 4, no statistics -- the unchanged
             schedule kind and the schedule sweep over --variants K variants: the four hourly rules with the thresholds,
             the limit and the grid-charge power scaled by factors spread over [0.6, 1.4] (the hold rule's thresholds stay
             at the range's end), variant v's array the hourly array rotated by v hours against the middle variant's.
             The middle variant is the schedule run itself: its table and soc are the schedule kind's bit for bit;
             columns 0-3 agree in every variant and every variant keeps the table's identities.  The yardstick is K x
             the schedule kind's median: ratio_sweep_k_schedule likewise.
Every run but the sweeps' has the same statistics beside its table.  The three launches of a battery-family table (map
pass, scan, replay pass) are timed separately as well (TMH_K_STORAGE_*), inside the TMH_K_EXPAND span.  The script
checks each run's variant and launch counts, the kind's identities (on the warm-up round's tables), that the
statistics of all runs agree bit for bit and that every table's ok seconds equal the histogram's count.  One warm-up
round, then --rounds timed ones.  Prints one JSON line: per run (and per launch) the milliseconds, their median, range
and spread (max / min), the ratio of every run to each run before it, for the whole expansion and per launch, the
kind's own keys and the device's name.  Needs a GPU (no fallback).  The script sets no time limit of its own: all
runs share one process (same code objects, same allocator), so the caller wraps it, e.g. `timeout -k 10 300 python
scripts/table_cost.py --kind demand`; a run that hangs ends the measurement, nothing is retried."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# per kind: the runs as (label in the JSON keys, what is enabled: None, a table, or "battery_fleet": the battery
# kind's table with the battery fleet series)
RUNS = {
    "intervals": (("stats_only", None), ("with_intervals", "intervals")),
    "registers": (("stats_only", None), ("intervals", "intervals"), ("registers", "registers")),
    "demand": (("stats_only", None), ("registers", "registers"), ("demand", "demand")),
    "storage": (("stats_only", None), ("registers", "registers"), ("storage", "storage")),
    "battery": (("stats_only", None), ("storage", "storage"), ("battery", "battery")),
    "battery_fleet": (("battery", "battery"), ("battery_fleet", "battery_fleet")),
    "battery_sweep": (("battery", "battery"), ("battery_sweep", "battery_sweep")),
    "dispatch": (("battery", "battery"), ("dispatch", "dispatch")),
    "dispatch_sweep": (("dispatch", "dispatch"), ("dispatch_sweep", "dispatch_sweep")),
    "schedule": (("dispatch", "dispatch"), ("schedule", "schedule")),
    "dispatch_fleet": (("dispatch", "dispatch"), ("dispatch_fleet", "dispatch_fleet")),
    "schedule_fleet": (("schedule", "schedule"), ("schedule_fleet", "schedule_fleet")),
    "schedule_sweep": (("schedule", "schedule"), ("schedule_sweep", "schedule_sweep")),
}
# the tables of the battery family (fp64 engines) and their three launches: _lib.K_STORAGE_<PART>
FAMILY = ("storage", "battery", "battery_fleet", "battery_sweep", "dispatch", "dispatch_sweep", "schedule", "dispatch_fleet",
          "schedule_fleet", "schedule_sweep")
PARTS = ("map", "scan", "replay")
SHORT = {"stats_only": "stats", "battery_fleet": "fleet", "dispatch_fleet": "fleet", "schedule_fleet": "fleet"}   # labels as the ratios' keys name them


def run_once(a, mp, stats, table, kw):
    """One engine run with `table` (RUNS) enabled with kw, statistics beside it if `stats`: the run's variant and
    launch counts checked; TMH_K_EXPAND's milliseconds, the launches' ({} outside the battery family) and their
    count, and the tensors the kinds' checks read."""
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    fleet = table is not None and table.endswith("_fleet")   # the kind's table with its fleet series beside it
    base = table[:-len("_fleet")] if fleet else table
    sim = BatchedSim(a.chains, a.start, tz="Europe/Berlin", params=mp, precision=a.precision, device="cuda:0", horizon=a.steps)
    if stats:
        sim.enable_stats()
    raw = getattr(sim, "enable_" + base)(a.steps, a.interval, **kw) if table else None
    fleet_rows = getattr(sim, "enable_battery_fleet" if base == "battery" else "enable_dispatch_fleet")(a.steps) if fleet else None
    _lib.check(sim.L.tmh_profile_enable(sim._eng, 1))
    sim.run(a.steps, trace=(), window=a.steps)
    torch.cuda.synchronize()
    ms, launches = _lib.profile_read(sim._eng, _lib.K_EXPAND)
    want = getattr(_lib, "OUT_" + (table or "stats").upper()) | (_lib.OUT_FP64 if a.precision == "fp64" else 0)
    assert launches == 1 and sim.L.tmh_engine_last_expand(sim._eng) == want, (launches, want)
    parts, groups = {}, None
    if table in FAMILY:   # its three launches, once each (a sweep: once per group of variants), inside the span read above
        counts = []
        for name in PARTS:
            parts[name], pn = _lib.profile_read(sim._eng, getattr(_lib, "K_STORAGE_" + name.upper()))
            counts.append(pn)
        groups = counts[0]
        assert counts == [groups] * 3 and (1 <= groups <= a.variants if table.endswith("_sweep") else groups == 1), counts
    if stats and raw is not None:
        assert int(raw[:, 2].sum()) == int(sim.hist.sum()) > 0
    return SimpleNamespace(ms=ms, parts=parts, groups=groups, raw=raw, fleet_rows=fleet_rows,
                           hist=sim.hist.clone() if stats else None, acc=sim.chain_acc.clone() if stats else None,
                           soc=sim.soc.clone() if sim.soc is not None else None)


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


# A kind's row, from the arguments `a` and the two battery settings (storage's, and `lossy` with the losses):
#   runs     (label, what is enabled, its enable_* arguments) per run, in the order they alternate
#   stats    whether the statistics run beside every table
#   check    the warm-up round's results (run_once, in the runs' order) -> the findings among the result's keys
#   keys     the setting among the result's keys
#   derived  (medians per label, per label and launch) -> the kind's own figures among the result's keys

def table_kind(a, battery, lossy):
    """The kinds measured over the statistics or over the table below them: check_tables' identities."""
    kw = {"storage": battery, "battery": lossy, "battery_fleet": lossy}
    runs = tuple((label, table, kw.get(table, {})) for label, table in RUNS[a.kind])

    def check(*rs):
        tables = {table: r.raw for (_, table, _), r in zip(runs, rs)}
        return dict(export_cells=check_tables(a.kind, {**tables, "fleet_rows": rs[-1].fleet_rows}, a.interval))

    def derived(med, pmed):
        if a.kind == "intervals":
            return dict(ratio=med["with_intervals"] / med["stats_only"],
                        ns_per_chain_second=[1e6 * med[label] / (a.chains * a.steps) for label, _, _ in runs])
        if a.kind == "storage":
            p = pmed["storage"]
            return dict(scan_share=p["scan"] / med["storage"], ratio_replay_registers=p["replay"] / med["registers"],
                        ratio_map_registers=p["map"] / med["registers"], scan_over_replay=p["scan"] / p["replay"])
        return {}

    keys = dict(modules=a.modules, battery=battery if a.kind == "storage" else lossy) if a.kind in FAMILY else {}
    return dict(runs=runs, stats=True, check=check, keys=keys, derived=derived)


def sweep_yardstick(K, kind, sweep):
    """The sweeps' derived figures: the sweep over K x the kind's median, for the whole expansion and per launch."""
    def derived(med, pmed):
        return dict(yardstick_ms=K * med[kind], sweep_ms_per_variant=med[sweep] / K,
                    **{f"ratio_sweep_k_{kind}": med[sweep] / (K * med[kind])},
                    **{f"ratio_{name}_sweep_k_{kind}": pmed[sweep][name] / (K * pmed[kind][name]) for name in PARTS})
    return derived


def battery_sweep_kind(a, battery, lossy):
    """The battery kind and the sweep over a.variants capacities."""
    K = a.variants
    caps = [a.capacity_wh * (0.8 + 0.4 * v / max(K - 1, 1)) for v in range(K)] if K > 1 else [a.capacity_wh]
    mid = (K - 1) // 2
    caps[mid] = a.capacity_wh
    soc0 = [c / 2 for c in caps]   # (half full, as the kind's: the variants differ from their first second)

    def check(bt, sw):   # the warm-up round's tables: the middle variant is the kind's, columns 0-3 every variant's
        import torch
        assert torch.equal(sw.raw[mid], bt.raw) and torch.equal(sw.soc[mid], bt.soc)
        for v in range(K):
            t = sw.raw[v]
            assert torch.equal(t[:, :4], bt.raw[:, :4]) and bool((t[:, 4:8] >= 0).all()) and bool((t[:, 9] >= 0).all())
            assert torch.equal(t[:, 4] - t[:, 5], t[:, 1] - t[:, 0] + t[:, 6] - t[:, 7])
            assert v == mid or not torch.equal(t[:, 4:], bt.raw[:, 4:])
        assert int(bt.raw[:, 6].sum()) > 0 and int(bt.raw[:, 7].sum()) > 0 and int(bt.raw[:, 9].sum()) > 0
        return dict(launch_groups=sw.groups)

    return dict(runs=(("battery", "battery", lossy),
                      ("battery_sweep", "battery_sweep", {**lossy, "capacity_wh": caps, "soc0_wh": soc0})),
                stats=False, check=check, keys=dict(modules=a.modules, battery=lossy, variants=K, capacities_wh=caps),
                derived=sweep_yardstick(K, "battery", "battery_sweep"))


def dispatch_kind(a, battery, lossy):
    """The battery kind and battery dispatch over the same batteries."""
    rule = dict(charge_above_w=a.charge_above_w, discharge_above_w=a.discharge_above_w, feed_in_limit_w=a.feed_in_limit_w)

    def check(bt, dp):   # the warm-up round's tables: the same seconds, the rule binds, the dispatch table's identities
        import torch
        b, d = bt.raw, dp.raw
        assert torch.equal(d[:, :4], b[:, :4]) and torch.equal(bt.hist, dp.hist)
        assert bool((d[:, 4:8] >= 0).all()) and bool((d[:, 9:11] >= 0).all())
        assert torch.equal(d[:, 4] - d[:, 5], d[:, 1] - d[:, 0] + d[:, 6] - d[:, 7] + d[:, 10])
        assert torch.equal(d[:, 11] != 0, d[:, 2] > 0) and torch.equal(d[:, 12] != 0, d[:, 2] > 0)
        lim = int(round(a.feed_in_limit_w * 4096))
        assert int((d[:, 12] >> 32).max()) == lim and int(d[:, 10].sum()) > 0                    # the limit binds
        assert 0 < int(d[:, 6].sum()) < int(b[:, 6].sum()) and 0 < int(d[:, 7].sum()) < int(b[:, 7].sum())   # the thresholds bind
        return dict(curtailed_share=int(d[:, 10].sum()) / int(d[:, 0].sum()), curtail_cells=int((d[:, 10] > 0).sum()),
                    charge_dispatch_over_battery=int(d[:, 6].sum()) / int(b[:, 6].sum()),
                    discharge_dispatch_over_battery=int(d[:, 7].sum()) / int(b[:, 7].sum()))

    return dict(runs=(("battery", "battery", lossy), ("dispatch", "dispatch", {**lossy, **rule})), stats=True, check=check,
                keys=dict(modules=a.modules, battery=lossy, rule=rule), derived=lambda med, pmed: {})


def dispatch_sweep_kind(a, battery, lossy):
    """The dispatch kind and the dispatch sweep over a.variants rule sets."""
    K = a.variants
    mid = (K - 1) // 2
    fac = [0.6 + 0.8 * v / (K - 1) for v in range(K)] if K > 1 else [1.0]
    fac[mid] = 1.0
    rule = dict(charge_above_w=a.charge_above_w, discharge_above_w=a.discharge_above_w, feed_in_limit_w=a.feed_in_limit_w)
    rules = {k: [w * f for f in fac] for k, w in rule.items()}

    def check(dp, sw):   # the warm-up round's tables: the middle variant is the kind's, columns 0-3 every variant's
        import torch
        assert torch.equal(sw.raw[mid], dp.raw) and torch.equal(sw.soc[mid], dp.soc)
        for v in range(K):
            t = sw.raw[v]
            assert torch.equal(t[:, :4], dp.raw[:, :4]) and bool((t[:, 4:8] >= 0).all()) and bool((t[:, 9:11] >= 0).all())
            assert torch.equal(t[:, 4] - t[:, 5], t[:, 1] - t[:, 0] + t[:, 6] - t[:, 7] + t[:, 10])
            assert torch.equal(t[:, 11] != 0, t[:, 2] > 0) and torch.equal(t[:, 12] != 0, t[:, 2] > 0)
            assert int((t[:, 12] >> 32).max()) == int(round(rules["feed_in_limit_w"][v] * 4096)) and int(t[:, 10].sum()) > 0
            assert v == mid or not torch.equal(t[:, 4:], dp.raw[:, 4:])
        d = dp.raw
        assert int(d[:, 6].sum()) > 0 and int(d[:, 7].sum()) > 0 and int(d[:, 9].sum()) > 0
        return dict(curtailed_shares=[int(sw.raw[v][:, 10].sum()) / int(d[:, 0].sum()) for v in range(K)],
                    launch_groups=sw.groups)

    return dict(runs=(("dispatch", "dispatch", {**lossy, **rule}),
                      ("dispatch_sweep", "dispatch_sweep", dict(n_variants=K, **lossy, **rules))),
                stats=False, check=check, keys=dict(modules=a.modules, battery=lossy, variants=K, rules=rules),
                derived=sweep_yardstick(K, "dispatch", "dispatch_sweep"))


def schedule_rules(a):
    """(dispatch's rule, the schedule's a.rules rule sets, the rule of each interval) of --rules 1 or 4."""
    import numpy as np
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
        sys.exit("--kind schedule, schedule_fleet: --rules 1 or 4")
    return rule, rules, roi


def schedule_kind(a, battery, lossy):
    """The dispatch kind and scheduled dispatch (a.rules rule sets) over the same batteries."""
    import numpy as np
    rule, rules, roi = schedule_rules(a)

    def check(dp, sc):   # the warm-up round's tables
        import torch
        d, s = dp.raw, sc.raw
        assert torch.equal(s[:, :4], d[:, :4]) and torch.equal(dp.hist, sc.hist)
        assert bool((s[:, 4:8] >= 0).all()) and bool((s[:, 9:11] >= 0).all())
        assert torch.equal(s[:, 4] - s[:, 5], s[:, 1] - s[:, 0] + s[:, 6] - s[:, 7] + s[:, 10])
        assert torch.equal(s[:, 11] != 0, s[:, 2] > 0) and torch.equal(s[:, 12] != 0, s[:, 2] > 0)
        assert int(d[:, 6].sum()) > 0 and int(d[:, 7].sum()) > 0 and int(d[:, 10].sum()) > 0
        if a.rules == 1:   # the same rule: the dispatch kind's bits
            assert torch.equal(s, d) and torch.equal(dp.soc, sc.soc)
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

    return dict(runs=(("dispatch", "dispatch", {**lossy, **rule}),
                      ("schedule", "schedule", dict(lossy, rules=rules, rule_of_interval=roi))),
                stats=True, check=check, derived=lambda med, pmed: {},
                keys=dict(modules=a.modules, battery=lossy, n_rules=a.rules, rules=rules, rule_of_interval=roi.tolist()))


def fleet_check(interval_s):
    """The dispatch fleet series' check on the warm-up round (the kind alone, the kind with the series): the same table
    and soc, the rows summed over each interval the table summed over the chains, and a fleet that curtails."""
    def check(alone, both):
        import torch
        t, fl = both.raw, both.fleet_rows
        assert torch.equal(alone.raw, t) and torch.equal(alone.soc, both.soc) and bool((fl[..., 4:] >= 0).all())
        if fl.shape[1] % interval_s == 0:
            per = fl[0].reshape(-1, interval_s, 9).sum(dim=1)
            for col, tcol in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (7, 6), (8, 10)):
                assert torch.equal(per[:, col], t[:, tcol].sum(dim=1)), (col, tcol)
        assert int(fl[..., 6].max()) > 0 and int(fl[..., 5].max()) > 0 and int(fl[..., 8].max()) > 0   # (a day's sum of [6] passes 2^63)
        return dict(export_cells=int((t[:, 5] > 0).sum()), curtail_seconds=int((fl[0, :, 8] > 0).sum()),
                    peak_fleet_import_w=int(fl[0, :, 4].max()) / 4096.0, peak_fleet_export_w=int(fl[0, :, 5].max()) / 4096.0)
    return check


def dispatch_fleet_kind(a, battery, lossy):
    """Battery dispatch alone and with the dispatch fleet series."""
    rule = dict(charge_above_w=a.charge_above_w, discharge_above_w=a.discharge_above_w, feed_in_limit_w=a.feed_in_limit_w)
    kw = {**lossy, **rule}
    return dict(runs=(("dispatch", "dispatch", kw), ("dispatch_fleet", "dispatch_fleet", kw)), stats=True,
                check=fleet_check(a.interval), keys=dict(modules=a.modules, battery=lossy, rule=rule), derived=lambda med, pmed: {})


def schedule_fleet_kind(a, battery, lossy):
    """The schedule (a.rules rule sets) alone and with the dispatch fleet series."""
    _, rules, roi = schedule_rules(a)
    kw = dict(lossy, rules=rules, rule_of_interval=roi)
    return dict(runs=(("schedule", "schedule", kw), ("schedule_fleet", "schedule_fleet", kw)), stats=True,
                check=fleet_check(a.interval), derived=lambda med, pmed: {},
                keys=dict(modules=a.modules, battery=lossy, n_rules=a.rules, rules=rules, rule_of_interval=roi.tolist()))


def schedule_sweep_kind(a, battery, lossy):
    """The schedule kind (four hourly rules) and the schedule sweep over a.variants scaled rule sets and rotated arrays."""
    import numpy as np
    K = a.variants
    mid = (K - 1) // 2
    fac = [0.6 + 0.8 * v / (K - 1) for v in range(K)] if K > 1 else [1.0]
    fac[mid] = 1.0
    if a.rules != 4:
        sys.exit("--kind schedule_sweep: --rules 4")
    _, rules, roi = schedule_rules(a)
    top = 32768.0   # the range's end (2^27 in the series' units): a hold rule's thresholds
    srules = [{k: [min(w * f, top) for f in fac] for k, w in rule.items()} for rule in rules]
    hours = np.arange(len(roi)) * a.interval // 3600
    arrays = np.stack([((hours + v - mid) % 4).astype(np.uint8) for v in range(K)])
    assert np.array_equal(arrays[mid], roi)

    def check(sc, sw):   # the warm-up round's tables: the middle variant is the kind's, columns 0-3 every variant's
        import torch
        assert torch.equal(sw.raw[mid], sc.raw) and torch.equal(sw.soc[mid], sc.soc)
        for v in range(K):
            t = sw.raw[v]
            assert torch.equal(t[:, :4], sc.raw[:, :4]) and bool((t[:, 4:8] >= 0).all()) and bool((t[:, 9:11] >= 0).all())
            assert torch.equal(t[:, 4] - t[:, 5], t[:, 1] - t[:, 0] + t[:, 6] - t[:, 7] + t[:, 10])
            assert torch.equal(t[:, 11] != 0, t[:, 2] > 0) and torch.equal(t[:, 12] != 0, t[:, 2] > 0)
            r = torch.from_numpy(arrays[v].astype(np.int64)).to(t.device)
            assert not bool(t[r == 1, 7].any()) and int(t[r == 1, 6].sum()) > 0      # the grid rule never discharges
            assert not bool(t[r == 2, 6].any()) and not bool(t[r == 2, 7].any())     # hold
            assert v == mid or not torch.equal(t[:, 4:], sc.raw[:, 4:])
        s = sc.raw
        assert int(s[:, 6].sum()) > 0 and int(s[:, 7].sum()) > 0 and int(s[:, 10].sum()) > 0
        return dict(import_over_schedule=[int(sw.raw[v][:, 4].sum()) / int(s[:, 4].sum()) for v in range(K)],
                    launch_groups=sw.groups)

    return dict(runs=(("schedule", "schedule", dict(lossy, rules=rules, rule_of_interval=roi)),
                      ("schedule_sweep", "schedule_sweep", dict(lossy, n_variants=K, rules=srules, rule_of_interval=arrays))),
                stats=False, check=check, derived=sweep_yardstick(K, "schedule", "schedule_sweep"),
                keys=dict(modules=a.modules, battery=lossy, variants=K, n_rules=a.rules, factors=fac, rules=rules,
                          rule_of_interval=roi.tolist()))


KINDS = {**{kind: table_kind for kind in RUNS}, "battery_sweep": battery_sweep_kind, "dispatch": dispatch_kind,
         "dispatch_sweep": dispatch_sweep_kind, "schedule": schedule_kind, "dispatch_fleet": dispatch_fleet_kind,
         "schedule_fleet": schedule_fleet_kind, "schedule_sweep": schedule_sweep_kind}


def assemble(a, row, t, pt, found, device, build_stamp):
    """The result: t {label: the rounds' ms}, pt {label: {launch: the rounds' ms}} ({} outside the battery family) and
    the check's findings beside the arguments and the row's own keys."""
    labels = [label for label, _, _ in row["runs"]]
    med = {k: statistics.median(t[k]) for k in labels}
    pmed = {k: {name: statistics.median(v) for name, v in pt[k].items()} for k in labels}
    res = dict(device=device, chains=a.chains, steps=a.steps, interval_s=a.interval, precision=a.precision, start=a.start,
               rounds=a.rounds, **row["keys"], **found)
    for k in labels:
        for key, v in [(k, t[k])] + [(f"{k}_{name}", v) for name, v in pt[k].items()]:
            res.update({f"{key}_ms": v, f"{key}_median_ms": statistics.median(v), f"{key}_range_ms": [min(v), max(v)],
                        f"{key}_spread": max(v) / min(v)})
    res["ns_per_chain_second"] = {k: 1e6 * med[k] / (a.chains * a.steps) for k in labels}
    for i, hi in enumerate(labels):   # every run over each run before it: the whole expansion, and each launch both have
        for lo in labels[:i]:
            pair = f"{SHORT.get(hi, hi)}_{SHORT.get(lo, lo)}"
            res[f"ratio_{pair}"] = med[hi] / med[lo]
            res.update({f"ratio_{name}_{pair}": pmed[hi][name] / pmed[lo][name] for name in pmed[hi] if name in pmed[lo]})
    res.update(row["derived"](med, pmed), build_stamp=build_stamp)
    return res


def parse_args(argv=None):
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
    ap.add_argument("--variants", type=int, default=5, help="--kind battery_sweep, dispatch_sweep, schedule_sweep: the variants per chain")
    ap.add_argument("--rules", type=int, default=1, help="--kind schedule, schedule_fleet: 1 (the dispatch kind's rule) or 4 hourly rules; schedule_sweep: 4")
    ap.add_argument("--charge-above-w", type=float, default=500.0, help="--kind dispatch: the charge threshold")
    ap.add_argument("--discharge-above-w", type=float, default=200.0, help="--kind dispatch: the discharge threshold")
    ap.add_argument("--feed-in-limit-w", type=float, default=1000.0, help="--kind dispatch: the feed-in limit")
    a = ap.parse_args(argv)
    if a.kind in FAMILY:
        a.precision = "fp64"   # (the kind's engines)
    return a


def kind_row(a):
    """The row of a.kind (KINDS) for the arguments' battery."""
    battery = dict(capacity_wh=a.capacity_wh, charge_w=a.charge_w, discharge_w=a.discharge_w, soc0_wh=a.capacity_wh / 2)
    lossy = dict(battery, charge_eff=a.charge_eff, discharge_eff=a.discharge_eff, standby_w=a.standby_w)
    return KINDS[a.kind](a, battery, lossy)


def main():
    a = parse_args()
    import torch
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.params import ModelParams
    if not torch.cuda.is_available():
        sys.exit("table_cost.py needs a GPU")
    mp = ModelParams()
    if a.modules != 1:   # k modules on a k-fold inverter
        import dataclasses
        mod, inv = dict(mp.module), dict(mp.inverter)
        mod["Impo"] *= a.modules
        for key in ("Paco", "Pdco", "Pso", "Pnt"):
            inv[key] *= a.modules
        inv["C0"] /= a.modules
        mp = dataclasses.replace(mp, module=mod, inverter=inv)
    row = kind_row(a)
    # warm-up (code objects, allocator), and the kind's check on its tables
    found = row["check"](*[run_once(a, mp, row["stats"], table, kw) for _, table, kw in row["runs"]])
    t ={label: [] for label, _, _ in row["runs"]}
    pt = {label: {} for label in t}
    ref = None
    for _ in range(a.rounds):
        for label, table, kw in row["runs"]:
            r = run_once(a, mp, row["stats"], table, kw)
            t[label].append(r.ms)
            for name, ms in r.parts.items():
                pt[label].setdefault(name, []).append(ms)
            if row["stats"]:
                ref = ref or (r.hist, r.acc)
                assert torch.equal(r.hist, ref[0]) and torch.equal(r.acc.view(torch.int64), ref[1].view(torch.int64))
            del r
    line = json.dumps(assemble(a, row, t, pt, found, torch.cuda.get_device_name(0), _lib.loaded_stamp()))
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
