"""scripts/table_cost.py's result assembly from fabricated timings: every key of the committed cost record of each kind
(profiles/*_cost.json) is among the keys produced, the setting's values are the record's, and the figures are the
arithmetic their names say.  No GPU: the script imports torch and the engine inside its functions."""
import importlib.util
import json
import os
import statistics

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("table_cost", os.path.join(ROOT, "scripts", "table_cost.py"))
table_cost = importlib.util.module_from_spec(spec)
spec.loader.exec_module(table_cost)

FAMILY = ["--modules", "20"]
# (record under profiles/, the arguments it was taken with, what the kind's check found -- fabricated, the record's keys)
RECORDS = {
    "intervals": ("intervals_cost.json", [], dict(export_cells=None)),
    "registers": ("registers_cost.json", [], dict(export_cells=7)),
    "demand": ("demand_cost.json", [], dict(export_cells=7)),
    "storage": ("storage_cost.json", FAMILY, dict(export_cells=7)),
    "battery": ("battery_cost.json", FAMILY, dict(export_cells=7)),
    "battery_fleet": ("battery_fleet_cost.json", FAMILY, dict(export_cells=7)),
    "battery_sweep": ("battery_sweep_cost.json", FAMILY, dict(launch_groups=2)),
    "dispatch": ("dispatch_cost.json", FAMILY, dict(curtailed_share=0.1, curtail_cells=3, charge_dispatch_over_battery=0.7,
                                                    discharge_dispatch_over_battery=0.8)),
    "dispatch_sweep": ("dispatch_sweep_cost.json", FAMILY, dict(curtailed_shares=[0.1] * 5, launch_groups=2)),
    "schedule": ("schedule_cost.json", FAMILY, dict(tables_equal=True)),
    "schedule-r4": ("schedule_cost_r4.json", FAMILY + ["--rules", "4"],
                    dict(tables_equal=False, differing_cells_import=5, import_schedule_over_dispatch=1.1,
                         charge_schedule_over_dispatch=1.8)),
}
# the setting: equal to the record's wherever the record has the key
SETTING = ("chains", "steps", "interval_s", "precision", "start", "rounds", "modules", "battery", "variants", "capacities_wh",
           "rule", "rules", "n_rules", "rule_of_interval")


def fabricated(case):
    record, argv, found = RECORDS[case]
    a = table_cost.parse_args(["--kind", case.split("-")[0]] + argv)
    row = table_cost.kind_row(a)
    labels = [label for label, _, _ in row["runs"]]
    t = {label: [10.0 * (i + 1) + r for r in (0.0, 2.0, 1.0)] for i, label in enumerate(labels)}   # two or three labels, three rounds
    pt = {label: {name: [ms * (j + 1) / 8 for ms in t[label]] for j, name in enumerate(table_cost.PARTS)}
          if table in table_cost.FAMILY else {} for label, table, _ in row["runs"]}
    res = json.loads(json.dumps(table_cost.assemble(a, row, t, pt, found, "a device", "a stamp")))
    with open(os.path.join(ROOT, "profiles", record)) as fh:
        return a, labels, t, pt, res, json.loads(fh.read())


@pytest.mark.parametrize("case", sorted(RECORDS))
def test_every_key_of_the_record_is_produced(case):
    a, labels, t, pt, res, record = fabricated(case)
    assert set(record) <= set(res), sorted(set(record) - set(res))
    for key in SETTING:
        if key in record:
            assert res[key] == record[key], key
    for key, value in RECORDS[case][2].items():
        assert res[key] == value
    assert res["device"] == "a device" and res["build_stamp"] == "a stamp"
    assert type(res["ns_per_chain_second"]) is type(record.get("ns_per_chain_second", {}))
    for label in labels:   # per run, and per launch of the battery family's
        for key, v in [(label, t[label])] + [(f"{label}_{name}", v) for name, v in pt[label].items()]:
            assert res[key + "_ms"] == v and res[key + "_median_ms"] == statistics.median(v)
            assert res[key + "_range_ms"] == [min(v), max(v)] and res[key + "_spread"] == max(v) / min(v)


def test_the_figures_are_what_their_names_say():
    med = lambda v: statistics.median(v)
    a, labels, t, pt, res, _ = fabricated("intervals")
    assert res["ratio"] == med(t["with_intervals"]) / med(t["stats_only"])
    assert res["ns_per_chain_second"] == [1e6 * med(t[k]) / (65536 * 86400) for k in labels]
    a, labels, t, pt, res, _ = fabricated("demand")
    assert res["ratio_demand_stats"] == med(t["demand"]) / med(t["stats_only"])
    assert res["ratio_demand_registers"] == med(t["demand"]) / med(t["registers"])
    assert res["ratio_registers_stats"] == med(t["registers"]) / med(t["stats_only"])
    assert res["ns_per_chain_second"]["demand"] == 1e6 * med(t["demand"]) / (65536 * 86400)
    a, labels, t, pt, res, _ = fabricated("storage")
    p = {name: med(v) for name, v in pt["storage"].items()}
    assert pt["registers"] == {} and "registers_map_ms" not in res
    assert res["scan_share"] == p["scan"] / med(t["storage"]) and res["scan_over_replay"] == p["scan"] / p["replay"]
    assert res["ratio_replay_registers"] == p["replay"] / med(t["registers"])
    assert res["ratio_map_registers"] == p["map"] / med(t["registers"])
    a, labels, t, pt, res, _ = fabricated("battery")
    assert res["ratio_battery_storage"] == med(t["battery"]) / med(t["storage"])
    assert res["ratio_scan_battery_storage"] == med(pt["battery"]["scan"]) / med(pt["storage"]["scan"])
    a, labels, t, pt, res, _ = fabricated("battery_fleet")
    assert res["ratio_fleet_battery"] == med(t["battery_fleet"]) / med(t["battery"])
    assert res["ratio_replay_fleet_battery"] == med(pt["battery_fleet"]["replay"]) / med(pt["battery"]["replay"])
    for case, kind, sweep in (("battery_sweep", "battery", "battery_sweep"), ("dispatch_sweep", "dispatch", "dispatch_sweep")):
        a, labels, t, pt, res, _ = fabricated(case)
        assert res["yardstick_ms"] == 5 * med(t[kind]) and res["sweep_ms_per_variant"] == med(t[sweep]) / 5
        assert res[f"ratio_sweep_k_{kind}"] == med(t[sweep]) / (5 * med(t[kind]))
        assert res[f"ratio_map_sweep_k_{kind}"] == med(pt[sweep]["map"]) / (5 * med(pt[kind]["map"]))
    a, labels, t, pt, res, _ = fabricated("schedule-r4")
    assert res["ratio_schedule_dispatch"] == med(t["schedule"]) / med(t["dispatch"])
    assert res["ratio_replay_schedule_dispatch"] == med(pt["schedule"]["replay"]) / med(pt["dispatch"]["replay"])
    assert len(res["rules"]) == 4 and res["rule_of_interval"][:9] == [0, 0, 0, 0, 1, 1, 1, 1, 2]
