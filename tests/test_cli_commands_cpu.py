"""The command-line surface of tmhpvsim_amd/cli.py, pinned parameter by parameter: the commands share their option
groups (the batch options, the battery's seven, dispatch's three, --interval / --all-chains), and a change to a
group must not move a name, an order, a default or a help text of any command.  The table below was recorded from
`main.commands[...].params` before the groups were folded into decorators.  No GPU."""
import os

import pytest

from tmhpvsim_amd import cli
from tmhpvsim_amd.cli import TABLE_CSV, main


def O(name, opts, help, default=None, required=False, multiple=False):
    return (name, tuple(opts.split()), required, default, multiple, help)


FILE = ("file", ("file",), True, None, False, None)
COMMON = [
    O("amqp_url", "--amqp-url", "AMQP URL (defaults to 'amqp://localhost:5672/')", os.environ.get("AMQP_URL")),
    O("exchange", "--exchange", "The name of the exchange (defaults to 'meter')", os.environ.get("TMHPVSIM_EXCHANGE", "meter")),
    O("verbose", "-v --verbose", "Increase logging level from default WARN", 0),
    O("realtime", "--realtime", "Switch off rate limiting (for simulation)", True),
    O("batch", "--batch", "offline engine mode: number of chains (site x scenario)"),
    O("start", "--start", "batch mode: local wall-clock start time", "2019-09-06T12:00:00"),
    O("seconds", "--seconds", "batch mode: seconds to simulate", 86400),
    O("seed", "--seed", "batch mode: keyed Philox seed", 24301),
]
# every command's parameters after FILE (metersim has none) and COMMON, in --help's order
COMMANDS = {
    "pvsim": [
        O("precision", "--precision", "batch mode arithmetic", "fp64"),
        O("all_chains", "--all-chains", "batch mode: also write every chain's traces to this .npz"),
    ],
    "metersim": [
        O("out_file", "--out", "batch mode: JSON-lines message file ('-' = stdout)", "-"),
    ],
    "fleet": [
        O("precision", "--precision", "batch mode arithmetic", "fp32"),
        O("bin_s", "--bin", "seconds per output row (a last partial bin is kept)", 1),
    ],
    "intervals": [
        O("precision", "--precision", "batch mode arithmetic", "fp32"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("all_chains", "--all-chains", "also write every chain's raw table and watt arrays to this .npz"),
    ],
    "registers": [
        O("precision", "--precision", "batch mode arithmetic", "fp32"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("all_chains", "--all-chains", "also write every chain's raw table and watt arrays to this .npz"),
    ],
    "demand": [
        O("precision", "--precision", "batch mode arithmetic", "fp32"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("all_chains", "--all-chains", "also write every chain's raw table and watt arrays to this .npz"),
    ],
    "storage": [
        O("all_chains", "--all-chains", "also write every chain's raw table and watt arrays to this .npz"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("capacity_wh", "--capacity-wh", "battery capacity (Wh)", required=True),
        O("charge_w", "--charge-w", "charge power limit (W)", required=True),
        O("discharge_w", "--discharge-w", "discharge power limit (W)", required=True),
        O("soc0_wh", "--soc0-wh", "every battery's state of charge at the start (Wh)", 0.0),
    ],
    "battery": [
        O("all_chains", "--all-chains", "also write every chain's raw table and watt arrays to this .npz"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("capacity_wh", "--capacity-wh", "battery capacity (Wh); a list is dealt to the chains", required=True),
        O("charge_w", "--charge-w", "charge power limit at the meter side (W)", required=True),
        O("discharge_w", "--discharge-w", "discharge power limit at the meter side (W)", required=True),
        O("charge_eff", "--charge-eff", "charge efficiency in [0.5, 1]", "1.0"),
        O("discharge_eff", "--discharge-eff", "discharge efficiency in [0.5, 1]", "1.0"),
        O("standby_w", "--standby-w", "standby drain (W)", "0.0"),
        O("soc0_wh", "--soc0-wh", "state of charge at the start (Wh)", "0.0"),
        O("fleet", "--fleet", "also write the battery fleet series' means per bin to this CSV"),
        O("bin_s", "--bin", "--fleet: seconds per row (a last partial bin is kept)", 1),
    ],
    "dispatch": [
        O("all_chains", "--all-chains", "also write every chain's raw table and watt arrays to this .npz"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("capacity_wh", "--capacity-wh", "battery capacity (Wh); a list is dealt to the chains", required=True),
        O("charge_w", "--charge-w", "charge power limit at the meter side (W)", required=True),
        O("discharge_w", "--discharge-w", "discharge power limit at the meter side (W)", required=True),
        O("charge_eff", "--charge-eff", "charge efficiency in [0.5, 1]", "1.0"),
        O("discharge_eff", "--discharge-eff", "discharge efficiency in [0.5, 1]", "1.0"),
        O("standby_w", "--standby-w", "standby drain (W)", "0.0"),
        O("soc0_wh", "--soc0-wh", "state of charge at the start (Wh)", "0.0"),
        O("charge_above_w", "--charge-above-w", "charge only from the surplus above this (W)", "0.0"),
        O("discharge_above_w", "--discharge-above-w", "discharge only into the deficit above this (W)", "0.0"),
        O("feed_in_limit_w", "--feed-in-limit-w", "feed-in limit (W); `none`: no limit (the default)"),
    ],
    "schedule": [
        O("all_chains", "--all-chains", "also write every chain's raw table and watt arrays to this .npz"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("capacity_wh", "--capacity-wh", "battery capacity (Wh); a list is dealt to the chains", required=True),
        O("charge_w", "--charge-w", "charge power limit at the meter side (W)", required=True),
        O("discharge_w", "--discharge-w", "discharge power limit at the meter side (W)", required=True),
        O("charge_eff", "--charge-eff", "charge efficiency in [0.5, 1]", "1.0"),
        O("discharge_eff", "--discharge-eff", "discharge efficiency in [0.5, 1]", "1.0"),
        O("standby_w", "--standby-w", "standby drain (W)", "0.0"),
        O("soc0_wh", "--soc0-wh", "state of charge at the start (Wh)", "0.0"),
        O("period", "--period", "HH:MM,CHARGE_ABOVE,DISCHARGE_ABOVE,LIMIT|none,GRID_CHARGE: a rule (watts) that starts daily at "
          "that local time; 1 to 8 of them", required=True, multiple=True),
    ],
    "battery-sweep": [
        O("all_chains", "--all-chains", "also write every variant's raw table of every chain to this .npz"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("capacity_wh", "--capacity-wh", "battery capacity (Wh); a list is one value per variant", required=True),
        O("charge_w", "--charge-w", "charge power limit at the meter side (W)", required=True),
        O("discharge_w", "--discharge-w", "discharge power limit at the meter side (W)", required=True),
        O("charge_eff", "--charge-eff", "charge efficiency in [0.5, 1]", "1.0"),
        O("discharge_eff", "--discharge-eff", "discharge efficiency in [0.5, 1]", "1.0"),
        O("standby_w", "--standby-w", "standby drain (W)", "0.0"),
        O("soc0_wh", "--soc0-wh", "state of charge at the start (Wh)", "0.0"),
    ],
    "dispatch-sweep": [
        O("all_chains", "--all-chains", "also write every variant's raw table of every chain to this .npz"),
        O("interval_s", "--interval", "seconds per metering interval (a last partial interval is kept)", 900),
        O("capacity_wh", "--capacity-wh", "battery capacity (Wh); a list is one value per variant", required=True),
        O("charge_w", "--charge-w", "charge power limit at the meter side (W)", required=True),
        O("discharge_w", "--discharge-w", "discharge power limit at the meter side (W)", required=True),
        O("charge_eff", "--charge-eff", "charge efficiency in [0.5, 1]", "1.0"),
        O("discharge_eff", "--discharge-eff", "discharge efficiency in [0.5, 1]", "1.0"),
        O("standby_w", "--standby-w", "standby drain (W)", "0.0"),
        O("soc0_wh", "--soc0-wh", "state of charge at the start (Wh)", "0.0"),
        O("charge_above_w", "--charge-above-w", "charge only from the surplus above this (W)", "0.0"),
        O("discharge_above_w", "--discharge-above-w", "discharge only into the deficit above this (W)", "0.0"),
        O("feed_in_limit_w", "--feed-in-limit-w", "feed-in limit (W); `none`: no limit (the default)"),
    ],
}
BATTERY_OPTIONS = ("capacity_wh", "charge_w", "discharge_w", "charge_eff", "discharge_eff", "standby_w", "soc0_wh")


def pinned(p):
    """(name, opts, required, default, multiple, help); a parameter without a default (click's own marker for it
    differs between releases) has None."""
    default = p.default if isinstance(p.default, (str, int, float)) else None
    return (p.name, tuple(p.opts), p.required, default, getattr(p, "multiple", False), getattr(p, "help", None))


def test_twelve_commands():
    assert sorted(main.commands) == sorted(COMMANDS) and len(COMMANDS) == 12


@pytest.mark.parametrize("name", sorted(COMMANDS))
def test_parameters_are_pinned(name):
    want = ([] if name == "metersim" else [FILE]) + COMMON + COMMANDS[name]
    got = [pinned(p) for p in main.commands[name].params]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w] or (len(got), len(want))


def test_battery_options_are_one_group():
    """The seven battery options are the same in the five commands that take lists -- type, callback and all --
    except for what the capacity's help says a list is."""
    def rows(name):
        ps = {p.name: p for p in main.commands[name].params}
        return [pinned(ps[o]) + (ps[o].callback, type(ps[o].type), ps[o].nargs, ps[o].is_flag) for o in BATTERY_OPTIONS]
    a_list_is = {"battery": "dealt to the chains", "dispatch": "dealt to the chains", "schedule": "dealt to the chains",
                 "battery-sweep": "one value per variant", "dispatch-sweep": "one value per variant"}
    head = "battery capacity (Wh); a list is "
    first = rows("battery")
    assert first[0][5] == head + a_list_is["battery"] and all(r[6] is not None for r in first)
    for name, words in a_list_is.items():
        got = rows(name)
        assert got[0][5] == head + words
        assert got[0][:5] + got[0][6:] == first[0][:5] + first[0][6:] and got[1:] == first[1:], name
    ps = {p.name: p for p in main.commands["dispatch"].params}
    qs = {p.name: p for p in main.commands["dispatch-sweep"].params}
    for o in ("charge_above_w", "discharge_above_w", "feed_in_limit_w"):
        assert pinned(ps[o]) + (ps[o].callback,) == pinned(qs[o]) + (qs[o].callback,) and ps[o].callback is not None


def test_table_csv_builds_on_itself():
    assert list(TABLE_CSV) == ["intervals", "registers", "demand", "storage", "battery", "dispatch", "schedule"]
    assert TABLE_CSV["schedule"] is TABLE_CSV["dispatch"] or TABLE_CSV["schedule"] == TABLE_CSV["dispatch"]
    assert TABLE_CSV["dispatch"][:9] == TABLE_CSV["battery"] and len(TABLE_CSV["dispatch"]) == 12
    assert [h for h, _ in TABLE_CSV["battery"]] == ["import_wh", "export_wh", "pv_wh", "meter_wh", "charge_wh", "discharge_wh",
                                                    "soc_wh", "loss_wh", "n_ok"]
    assert TABLE_CSV["battery"][:7] == TABLE_CSV["storage"][:7] and TABLE_CSV["battery"][8] == TABLE_CSV["storage"][7]
    assert TABLE_CSV["demand"][:6] == TABLE_CSV["registers"] == cli.REGISTERS_CSV
