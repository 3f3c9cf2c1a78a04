"""`pvsim` / `metersim` entry points with the reference's options plus a batched
offline mode that drives the MI355X engine (tmhpvsim/pvsim.py:103-121,
tmhpvsim/metersim.py:79-95).

    python -m tmhpvsim_amd.cli pvsim FILE [--amqp-url URL] [--exchange NAME] [-v]
                                          [--realtime/--no-realtime]
                                          [--batch N --start T --seconds S --seed K
                                           --precision fp64|fp32 --all-chains OUT.npz]
    python -m tmhpvsim_amd.cli metersim [--amqp-url URL] [--exchange NAME] [-v]
                                        [--realtime/--no-realtime]
                                        [--batch N --start T --seconds S --seed K --out FILE]
    python -m tmhpvsim_amd.cli fleet FILE --batch N --no-realtime [--bin S] [--precision fp32|fp64]
                                          [--start T --seconds S --seed K]
    python -m tmhpvsim_amd.cli intervals FILE --batch N --no-realtime --interval S [--all-chains NPZ]
                                              [--precision fp32|fp64] [--start T --seconds S --seed K]
    python -m tmhpvsim_amd.cli registers FILE --batch N --no-realtime --interval S [--all-chains NPZ]
                                              [--precision fp32|fp64] [--start T --seconds S --seed K]
    python -m tmhpvsim_amd.cli demand FILE --batch N --no-realtime --interval S [--all-chains NPZ]
                                           [--precision fp32|fp64] [--start T --seconds S --seed K]
    python -m tmhpvsim_amd.cli storage FILE --batch N --no-realtime --interval S --capacity-wh X --charge-w P
                                            --discharge-w P [--soc0-wh X] [--all-chains NPZ]
                                            [--start T --seconds S --seed K]
    python -m tmhpvsim_amd.cli battery FILE --batch N --no-realtime --interval S --capacity-wh X[,X..] --charge-w P[,P..]
                                            --discharge-w P[,P..] [--charge-eff E[,E..]] [--discharge-eff E[,E..]]
                                            [--standby-w P[,P..]] [--soc0-wh X[,X..]] [--all-chains NPZ]
                                            [--fleet CSV [--bin S]] [--start T --seconds S --seed K]
    python -m tmhpvsim_amd.cli dispatch FILE --batch N --no-realtime --interval S <the battery command's options>
                                             [--charge-above-w P[,P..]] [--discharge-above-w P[,P..]]
                                             [--feed-in-limit-w P|none[,..]] [--all-chains NPZ]
    python -m tmhpvsim_amd.cli schedule FILE --batch N --no-realtime --interval S <the battery command's options>
                                             --period HH:MM,CHARGE_ABOVE,DISCHARGE_ABOVE,LIMIT|none,GRID_CHARGE
                                             [--period ...] [--all-chains NPZ]

Without --batch the commands are the reference's AMQP pipelines (a fanout
exchange carrying one JSON float per second, pvsim.py:43-84, metersim.py:13-62):
they need aio_pika and a broker and are not rebuilt here (out of scope);
the command says so and exits non-zero.

--batch N --no-realtime is the offline mode: N chains (site x scenario) advance
on the GPU for --seconds seconds from --start in one engine run, with the meter
draw fused into the kernel.  `pvsim` writes FILE exactly like the reference's
write_file (pvsim.py:72-84: header `time,meter,pv,residual load`, one row per
second, residual = meter - pv) for chain 0, and optionally every chain's traces
to an .npz.  `metersim` writes the messages it would publish, one JSON object per
line: {"timestamp": ..., "body": <json.dumps(meter)>} (metersim.py:38-42).
`fleet` runs N chains series-only (no per-chain trace leaves the GPU, so N may be
large) and writes the fleet's means per bin of --bin seconds: header
`time,n_ok,meter,pv,residual load,covered` -- the bin's start, its ok chain-seconds,
the mean meter, pv and residual load per ok chain-second (W) and the share of them
under cloud (tmhpvsim_amd.series).
`intervals` runs N chains with interval metering only (tmhpvsim_amd.intervals: each
chain's exact energy per metering interval of --interval seconds; no per-second trace
leaves the GPU) and writes the reference's CSV columns `time,meter,pv,residual load` as
interval means for chain 0, one row per interval stamped with the interval's start;
--all-chains writes every chain's raw table and its watt / watt-hour arrays to an .npz.
`registers` runs N chains with the import / export registers only (tmhpvsim_amd.registers:
what each chain's bidirectional meter reads per interval of --interval seconds) and writes
chain 0's intervals: header `time,import_wh,export_wh,pv_wh,meter_wh,self_wh,n_ok` -- the
interval's start, the energy drawn from the grid, fed in, produced, consumed and
self-consumed (Wh) and the ok seconds; --all-chains writes every chain's raw table and
its watt / watt-hour arrays and ratios to an .npz.
`demand` runs N chains with the demand registers only (tmhpvsim_amd.demand: the registers
plus each interval's peak import and peak feed-in and when each happened) and writes chain
0's intervals: the `registers` columns plus `peak_import_w,t_peak_import_s,peak_export_w,
t_peak_export_s` -- the highest power drawn from the grid and fed in (W) and the earliest
second of the interval at which each occurred; --all-chains writes every chain's raw table
and its arrays to an .npz.
`storage` runs N chains with a battery behind each meter (tmhpvsim_amd.storage: capacity
--capacity-wh, power limits --charge-w and --discharge-w, every battery starting at --soc0-wh;
greedy self-consumption, lossless; an fp64 engine run) and writes chain 0's intervals: header
`time,import_wh,export_wh,pv_wh,meter_wh,charge_wh,discharge_wh,soc_wh,n_ok` -- the energy
drawn from the grid and fed in with the battery, produced, consumed, put into and taken out of
the battery (Wh), the state of charge at the interval's end and the ok seconds; --all-chains
writes every chain's raw table and its arrays to an .npz.
`battery` is `storage` with losses and per-chain batteries (tmhpvsim_amd.battery: charge and
discharge efficiency in [0.5, 1], a standby drain in W).  Each battery option takes one value or a
comma-separated list dealt to the chains round-robin (chain i gets value i mod the list's length):
a fleet of different batteries, or a sweep of sizes across otherwise equal scenarios in one run.
The CSV is `storage`'s with `loss_wh` (conversion and standby losses) before `n_ok`; --all-chains
writes every chain's raw table and its arrays to an .npz.  --fleet CSV also writes the battery fleet series
(tmhpvsim_amd.battery.fleet_to_watts: what the whole batch does second by second behind its batteries) as means
per ok chain-second over bins of --bin seconds: header `time,n_ok,meter,pv,import_w,export_w,charge_w,discharge_w,
soc_wh,covered`; without it the command's outputs are as before, byte for byte.
`dispatch` is `battery` under thresholds and a feed-in limit (tmhpvsim_amd.dispatch): the battery charges only
from the surplus above --charge-above-w, discharges only into the deficit above --discharge-above-w, and what is
left of the surplus is fed in up to --feed-in-limit-w (`none`, the default: no limit), the rest curtailed.  Lists
are dealt round-robin as `battery` deals them.  The CSV is `battery`'s with `curtailed_wh,peak_import_w,
peak_export_w` after `n_ok` (export_wh is what was fed in after the limit, pv_wh the available PV); --all-chains
writes every chain's raw table and its arrays to an .npz.
`schedule` is `dispatch` under a daily tariff (tmhpvsim_amd.schedule): each --period starts a rule -- the two
thresholds, the feed-in limit (`none`: no limit) and the power the battery also takes from the grid, in watts -- daily
at that local time (1 to 8 of them; an interval that contains a period's start still belongs to the period before).
The CSV is `dispatch`'s with a last column `rule`, the index of the --period in force in the interval; --all-chains
writes every chain's raw table, its arrays and `rule` to an .npz.
There is no CPU fallback: the batch mode fails if the engine cannot run.
"""
from __future__ import annotations

import contextlib
import csv
import datetime as dt
import json
import logging
import os

import click

logger = logging.getLogger(__name__)


def _open_sim(n, start, seconds, seed, precision):
    """The batch mode's engine: n chains from `start` with a horizon of `seconds`, or the refusal without a GPU."""
    from .engine import BatchedSim
    from .params import ModelParams
    import torch
    if not torch.cuda.is_available():
        raise click.ClickException("--batch runs on the MI355X engine and no GPU is visible (there is no CPU path)")
    params = ModelParams(seed=int(seed))
    return BatchedSim(int(n), start, tz=params.site.tz, params=params, precision=precision, device="cuda:0",
                      horizon=int(seconds))


def _warn_faulted(sim, n, what):
    bad = int((sim.status() != 0).sum())
    if bad:
        logger.warning(f"{bad} of {n} chains faulted (reference exceptions); {what}")


@contextlib.contextmanager
def _refusals():
    """A ValueError inside the block (a quantity outside its range: the kind's quantize_params and its like) is the
    command's refusal."""
    try:
        yield
    except ValueError as e:
        raise click.ClickException(str(e))


def _batch_run(n, start, seconds, seed, precision, fields):
    import torch
    sim = _open_sim(n, start, seconds, seed, precision)
    out = sim.run(int(seconds), trace=fields)
    torch.cuda.synchronize()
    _warn_faulted(sim, n, "their values are NaN")
    return {k: v.double().cpu().numpy() if v.dtype != torch.uint8 else v.cpu().numpy() for k, v in out.items()}


def _fleet_run(n, start, seconds, seed, precision, bin_s):
    sim = _open_sim(n, start, seconds, seed, precision)
    sim.enable_series(int(seconds))
    sim.run(int(seconds), trace=())
    out = sim.series(bin_s=int(bin_s), mean=True)
    _warn_faulted(sim, n, "the means are over the ok chains")
    return {k: v[0] for k, v in out.items()}


def _table_run(kind, n, start, seconds, seed, precision, interval_s, fleet_bin=None, **enable_kw):
    """An engine run with the interval table `kind` ("intervals", "registers", "demand", "storage", "battery", "dispatch" or "schedule")
    only: the raw table, its watt / watt-hour arrays and, with fleet_bin (the battery kind), the battery fleet
    series' means per bin of fleet_bin seconds (else None).  enable_kw: the kind's own arguments."""
    sim = _open_sim(n, start, seconds, seed, precision)
    raw = getattr(sim, "enable_" + kind)(int(seconds), int(interval_s), **enable_kw)
    if fleet_bin:
        sim.enable_battery_fleet(int(seconds))
    sim.run(int(seconds), trace=())
    out = getattr(sim, kind)()
    fleet = {k: v[0] for k, v in sim.battery_fleet(bin_s=int(fleet_bin), mean=True).items()} if fleet_bin else None
    _warn_faulted(sim, n, f"their {'intervals' if kind == 'intervals' else 'registers'} hold the seconds before the fault")
    return raw.cpu().numpy(), out, fleet


def _times(start, seconds):
    t0 = dt.datetime.fromisoformat(str(start))
    return [t0 + dt.timedelta(seconds=s) for s in range(int(seconds))]


def _batch_mode(verbose, realtime, batch, name):
    """What every command begins with: the logging level, then the refusal of anything but the offline mode."""
    logging.basicConfig(level=logging.WARN - 10 * verbose)
    if batch is None:
        try:
            import aio_pika  # noqa: F401
        except ImportError:
            raise click.ClickException(
                f"{name} without --batch is the reference's AMQP pipeline (aio_pika + a broker), which is not part of "
                "this build; use --batch N --no-realtime for the offline engine mode")
        raise click.ClickException(f"{name}: the AMQP pipeline is out of scope here; use --batch N --no-realtime")
    if realtime:
        raise click.ClickException("--batch is an offline mode: combine it with --no-realtime")


def _options(*opts):
    """The options as one decorator; --help lists them in the order given."""
    def decorate(f):
        for opt in reversed(opts):
            f = opt(f)
        return f
    return decorate


common = _options(
    click.option("--amqp-url", default=os.environ.get("AMQP_URL"), help="AMQP URL (defaults to 'amqp://localhost:5672/')"),
    click.option("--exchange", default=os.environ.get("TMHPVSIM_EXCHANGE", "meter"),
                 help="The name of the exchange (defaults to 'meter')"),
    click.option("-v", "--verbose", count=True, help="Increase logging level from default WARN"),
    click.option("--realtime/--no-realtime", default=True, help="Switch off rate limiting (for simulation)"),
    click.option("--batch", type=int, default=None, help="offline engine mode: number of chains (site x scenario)"),
    click.option("--start", default="2019-09-06T12:00:00", help="batch mode: local wall-clock start time"),
    click.option("--seconds", type=int, default=86400, help="batch mode: seconds to simulate"),
    click.option("--seed", type=int, default=0x5EED, help="batch mode: keyed Philox seed"))


@click.group()
def main():
    """tmhpvsim entry points on the MI355X engine."""


@main.command()
@click.argument("file")
@common
@click.option("--precision", type=click.Choice(["fp64", "fp32"]), default="fp64", help="batch mode arithmetic")
@click.option("--all-chains", default=None, help="batch mode: also write every chain's traces to this .npz")
def pvsim(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, precision, all_chains):
    """Simulated PV + meter + residual load to FILE (CSV, pvsim.py:72-84)."""
    _batch_mode(verbose, realtime, batch, "pvsim")
    out = _batch_run(batch, start, seconds, seed, precision, ("meter", "pv", "residual"))
    with open(file, mode="w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["time", "meter", "pv", "residual load"])
        m, p, r = out["meter"][:, 0], out["pv"][:, 0], out["residual"][:, 0]
        for i, t in enumerate(_times(start, seconds)):
            w.writerow([t, float(m[i]), float(p[i]), float(r[i])])
    if all_chains:
        import numpy as np
        np.savez(all_chains, **out)
    click.echo(f"wrote {seconds} rows to {file}" + (f" and {batch} chains to {all_chains}" if all_chains else ""))


@main.command()
@common
@click.option("--out", "out_file", default="-", help="batch mode: JSON-lines message file ('-' = stdout)")
def metersim(amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, out_file):
    """Meter values as the AMQP messages of metersim.py:38-42, one JSON object per line."""
    _batch_mode(verbose, realtime, batch, "metersim")
    out = _batch_run(batch, start, seconds, seed, "fp64", ("meter",))
    m = out["meter"]
    with click.open_file(out_file, "w") as fh:
        for i, t in enumerate(_times(start, seconds)):
            for c in range(m.shape[1]):
                rec = {"timestamp": t.isoformat(), "body": json.dumps(float(m[i, c]), ensure_ascii=False)}
                if m.shape[1] > 1:
                    rec["chain"] = c
                fh.write(json.dumps(rec) + "\n")


@main.command()
@click.argument("file")
@common
@click.option("--precision", type=click.Choice(["fp64", "fp32"]), default="fp32", help="batch mode arithmetic")
@click.option("--bin", "bin_s", type=click.IntRange(min=1), default=1, help="seconds per output row (a last partial bin is kept)")
def fleet(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, precision, bin_s):
    """Fleet means per bin over --batch chains to FILE (CSV; series-only engine run)."""
    _batch_mode(verbose, realtime, batch, "fleet")
    out = _fleet_run(batch, start, seconds, seed, precision, bin_s)
    t0 = dt.datetime.fromisoformat(str(start))
    with open(file, mode="w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["time", "n_ok", "meter", "pv", "residual load", "covered"])
        for i in range(len(out["n_ok"])):
            w.writerow([t0 + dt.timedelta(seconds=i * bin_s), int(out["n_ok"][i]), float(out["meter"][i]),
                        float(out["pv"][i]), float(out["residual"][i]), float(out["covered"][i])])
    click.echo(f"wrote {len(out['n_ok'])} rows to {file}")


REGISTERS_CSV = (("import_wh", "energy_wh_import"), ("export_wh", "energy_wh_export"), ("pv_wh", "energy_wh_pv"),
                 ("meter_wh", "energy_wh_meter"), ("self_wh", "energy_wh_self"), ("n_ok", "n_ok"))
# chain 0's CSV columns per interval table: (header, key of the table's watt / watt-hour arrays)
TABLE_CSV = {
    "intervals": (("meter", "meter"), ("pv", "pv"), ("residual load", "residual")),
    "registers": REGISTERS_CSV,
    "demand": REGISTERS_CSV + (("peak_import_w", "peak_import"), ("t_peak_import_s", "t_peak_import"),
                               ("peak_export_w", "peak_export"), ("t_peak_export_s", "t_peak_export")),
    "storage": (("import_wh", "energy_wh_import"), ("export_wh", "energy_wh_export"), ("pv_wh", "energy_wh_pv"),
                ("meter_wh", "energy_wh_meter"), ("charge_wh", "energy_wh_charge"), ("discharge_wh", "energy_wh_discharge"),
                ("soc_wh", "soc_wh"), ("n_ok", "n_ok")),
}
# (each later kind of the battery family holds the earlier one's columns: battery's loss goes before n_ok)
TABLE_CSV["battery"] = TABLE_CSV["storage"][:-1] + (("loss_wh", "energy_wh_loss"),) + TABLE_CSV["storage"][-1:]
TABLE_CSV["dispatch"] = TABLE_CSV["battery"] + (("curtailed_wh", "energy_wh_curtailed"), ("peak_import_w", "peak_w_import"),
                                                ("peak_export_w", "peak_w_export"))
TABLE_CSV["schedule"] = TABLE_CSV["dispatch"]   # (and the command's own last column, `rule`)

# the battery fleet series' CSV columns: (header, key of battery.fleet_to_watts)
FLEET_CSV = (("n_ok", "n_ok"), ("meter", "meter"), ("pv", "pv"), ("import_w", "import_w"), ("export_w", "export_w"),
             ("charge_w", "charge_w"), ("discharge_w", "discharge_w"), ("soc_wh", "soc_wh"), ("covered", "covered"))


def _table_command(kind, file, batch, start, seconds, seed, precision, interval_s, all_chains, fleet=None, bin_s=1,
                   csv_extra=None, **enable_kw):
    """The `intervals`, `registers`, `demand`, `storage`, `battery`, `dispatch` and `schedule` commands: chain 0's rows to
    FILE, every chain to the .npz; with `fleet` (the battery command's --fleet) the battery fleet series' means per bin
    to that CSV.  csv_extra: {header: one value per interval}, columns after the kind's (and arrays of the .npz)."""
    csv_extra = csv_extra or {}
    raw, out, fl = _table_run(kind, batch, start, seconds, seed, precision, interval_s,
                              fleet_bin=bin_s if fleet else None, **enable_kw)
    t0 = dt.datetime.fromisoformat(str(start))
    rows = raw.shape[0]
    with open(file, mode="w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["time"] + [name for name, _ in TABLE_CSV[kind]] + list(csv_extra))
        for k in range(rows):
            w.writerow([t0 + dt.timedelta(seconds=k * interval_s)] + [float(out[key][k, 0]) for _, key in TABLE_CSV[kind]]
                       + [int(v[k]) for v in csv_extra.values()])
    if all_chains:
        import numpy as np
        np.savez(all_chains, raw=raw, interval_s=interval_s, **out, **csv_extra)
    if fleet:
        with open(fleet, mode="w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["time"] + [name for name, _ in FLEET_CSV])
            for i in range(len(fl["n_ok"])):
                w.writerow([t0 + dt.timedelta(seconds=i * bin_s)] + [float(fl[key][i]) for _, key in FLEET_CSV])
    click.echo(f"wrote {rows} rows to {file}" + (f" and {batch} chains to {all_chains}" if all_chains else "")
               + (f" and {len(fl['n_ok'])} fleet rows to {fleet}" if fleet else ""))


def table_options(precision=True, every="chain's raw table and watt arrays"):
    """--interval and --all-chains (`every`: what the .npz holds), after --precision unless the command is fp64 only."""
    all_chains = click.option("--all-chains", default=None, help=f"also write every {every} to this .npz")
    interval = click.option("--interval", "interval_s", type=click.IntRange(min=1), default=900,
                            help="seconds per metering interval (a last partial interval is kept)")
    if not precision:
        return _options(all_chains, interval)
    return _options(click.option("--precision", type=click.Choice(["fp64", "fp32"]), default="fp32", help="batch mode arithmetic"),
                    interval, all_chains)


@main.command()
@click.argument("file")
@common
@table_options()
def intervals(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, precision, interval_s, all_chains):
    """Interval means of chain 0 over --batch chains to FILE (CSV; interval-metering engine run)."""
    _batch_mode(verbose, realtime, batch, "intervals")
    _table_command("intervals", file, batch, start, seconds, seed, precision, interval_s, all_chains)


@main.command()
@click.argument("file")
@common
@table_options()
def registers(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, precision, interval_s, all_chains):
    """Import / export registers of chain 0 over --batch chains to FILE (CSV; registers-only engine run)."""
    _batch_mode(verbose, realtime, batch, "registers")
    _table_command("registers", file, batch, start, seconds, seed, precision, interval_s, all_chains)


@main.command()
@click.argument("file")
@common
@table_options()
def demand(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, precision, interval_s, all_chains):
    """Demand registers of chain 0 over --batch chains to FILE (CSV; demand-only engine run)."""
    _batch_mode(verbose, realtime, batch, "demand")
    _table_command("demand", file, batch, start, seconds, seed, precision, interval_s, all_chains)


@main.command()
@click.argument("file")
@common
@table_options(precision=False)
@click.option("--capacity-wh", type=float, required=True, help="battery capacity (Wh)")
@click.option("--charge-w", type=float, required=True, help="charge power limit (W)")
@click.option("--discharge-w", type=float, required=True, help="discharge power limit (W)")
@click.option("--soc0-wh", type=float, default=0.0, help="every battery's state of charge at the start (Wh)")
def storage(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, interval_s, all_chains, capacity_wh,
            charge_w, discharge_w, soc0_wh):
    """Battery storage of chain 0 over --batch chains to FILE (CSV; storage-only fp64 engine run)."""
    _batch_mode(verbose, realtime, batch, "storage")
    _table_command("storage", file, batch, start, seconds, seed, "fp64", interval_s, all_chains, capacity_wh=capacity_wh,
                   charge_w=charge_w, discharge_w=discharge_w, soc0_wh=soc0_wh)


def _dealt(ctx, param, value):
    """A battery option: one float or a comma-separated list of them."""
    try:
        vals = [float(v) for v in str(value).split(",")]
    except ValueError:
        raise click.BadParameter("a number or a comma-separated list of numbers")
    return vals


def _dealt_limit(ctx, param, value):
    """--feed-in-limit-w: one value or a comma-separated list, each a number of watts or `none` (no limit)."""
    if value is None:
        return [None]
    try:
        return [None if v.strip().lower() == "none" else float(v) for v in str(value).split(",")]
    except ValueError:
        raise click.BadParameter("a number, `none`, or a comma-separated list of them")


def battery_options(a_list_is):
    """The battery's seven options; a_list_is: what a command does with a comma-separated list."""
    return _options(
        click.option("--capacity-wh", callback=_dealt, required=True, help=f"battery capacity (Wh); a list is {a_list_is}"),
        click.option("--charge-w", callback=_dealt, required=True, help="charge power limit at the meter side (W)"),
        click.option("--discharge-w", callback=_dealt, required=True, help="discharge power limit at the meter side (W)"),
        click.option("--charge-eff", callback=_dealt, default="1.0", help="charge efficiency in [0.5, 1]"),
        click.option("--discharge-eff", callback=_dealt, default="1.0", help="discharge efficiency in [0.5, 1]"),
        click.option("--standby-w", callback=_dealt, default="0.0", help="standby drain (W)"),
        click.option("--soc0-wh", callback=_dealt, default="0.0", help="state of charge at the start (Wh)"))


dispatch_options = _options(
    click.option("--charge-above-w", callback=_dealt, default="0.0", help="charge only from the surplus above this (W)"),
    click.option("--discharge-above-w", callback=_dealt, default="0.0", help="discharge only into the deficit above this (W)"),
    click.option("--feed-in-limit-w", callback=_dealt_limit, default=None, help="feed-in limit (W); `none`: no limit (the default)"))


def _deal(vals, n):
    """vals dealt to n chains round-robin."""
    return [vals[i % len(vals)] for i in range(int(n))]


def _dealt_table_command(kind, file, batch, start, seconds, seed, interval_s, all_chains, lists, **kw):
    """_table_command for the fp64 kinds whose option `lists` (a list per battery or dispatch option) are dealt to the
    chains; a quantity outside its range (the kind's quantize_params) is the command's refusal."""
    with _refusals():
        _table_command(kind, file, batch, start, seconds, seed, "fp64", interval_s, all_chains,
                       **{k: _deal(v, batch) for k, v in lists.items()}, **kw)


@main.command()
@click.argument("file")
@common
@table_options(precision=False)
@battery_options("dealt to the chains")
@click.option("--fleet", default=None, help="also write the battery fleet series' means per bin to this CSV")
@click.option("--bin", "bin_s", type=click.IntRange(min=1), default=1, help="--fleet: seconds per row (a last partial bin is kept)")
def battery(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, interval_s, all_chains, fleet, bin_s, **lists):
    """Battery storage with losses of chain 0 over --batch chains to FILE (CSV; battery-only fp64 engine run)."""
    _batch_mode(verbose, realtime, batch, "battery")
    _dealt_table_command("battery", file, batch, start, seconds, seed, interval_s, all_chains, lists, fleet=fleet, bin_s=bin_s)


@main.command()
@click.argument("file")
@common
@table_options(precision=False)
@battery_options("dealt to the chains")
@dispatch_options
def dispatch(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, interval_s, all_chains, **lists):
    """Battery dispatch (thresholds, a feed-in limit) of chain 0 over --batch chains to FILE (CSV; fp64 engine run)."""
    _batch_mode(verbose, realtime, batch, "dispatch")
    _dealt_table_command("dispatch", file, batch, start, seconds, seed, interval_s, all_chains, lists)


def parse_period(text):
    """One --period of the schedule command, HH:MM,CHARGE_ABOVE,DISCHARGE_ABOVE,LIMIT|none,GRID_CHARGE (watts): the
    period's start in seconds after local midnight and its rule as schedule.quantize_params takes it.  ValueError
    naming the period on anything else."""
    parts = [p.strip() for p in str(text).split(",")]
    try:
        if len(parts) != 5:
            raise ValueError("five fields")
        hh, mm = parts[0].split(":")
        if not (hh.isdigit() and mm.isdigit() and 0 <= int(hh) < 24 and 0 <= int(mm) < 60):
            raise ValueError("HH:MM")
        lim = None if parts[3].lower() == "none" else float(parts[3])
        rule = dict(charge_above_w=float(parts[1]), discharge_above_w=float(parts[2]), feed_in_limit_w=lim,
                    grid_charge_w=float(parts[4]))
    except ValueError:
        raise ValueError(f"--period {text!r}: expected HH:MM,CHARGE_ABOVE,DISCHARGE_ABOVE,LIMIT|none,GRID_CHARGE")
    return int(hh) * 3600 + int(mm) * 60, rule


def _period(ctx, param, value):
    try:
        return [parse_period(v) for v in value]
    except ValueError as e:
        raise click.BadParameter(str(e))


@main.command()
@click.argument("file")
@common
@table_options(precision=False)
@battery_options("dealt to the chains")
@click.option("--period", multiple=True, required=True, callback=_period,
              help="HH:MM,CHARGE_ABOVE,DISCHARGE_ABOVE,LIMIT|none,GRID_CHARGE: a rule (watts) that starts daily at that local "
                   "time; 1 to 8 of them")
def schedule(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, interval_s, all_chains, period, **lists):
    """Scheduled dispatch (a daily tariff of rules, grid charging) of chain 0 over --batch chains to FILE (CSV with the
    rule of each interval; fp64 engine run)."""
    _batch_mode(verbose, realtime, batch, "schedule")
    from . import schedule as S
    from .params import ModelParams
    if not 1 <= len(period) <= S.RULES_MAX:
        raise click.ClickException(f"schedule: {len(period)} --period options outside [1, {S.RULES_MAX}]")
    with _refusals():   # (two periods at one time: schedule.daily)
        rule_of_interval = S.daily(start, ModelParams(seed=int(seed)).site.tz, int(seconds), int(interval_s),
                                   [(s, r) for r, (s, _) in enumerate(period)])
    _dealt_table_command("schedule", file, batch, start, seconds, seed, interval_s, all_chains, lists,
                         csv_extra={"rule": rule_of_interval}, rules=[rule for _, rule in period],
                         rule_of_interval=rule_of_interval)


SWEEP_OPTIONS = ("capacity_wh", "charge_w", "discharge_w", "charge_eff", "discharge_eff", "standby_w", "soc0_wh")
# the battery-sweep CSV: a row per variant -- its parameters, then (header, key of battery.sweep_summary) fleet totals
# (Wh summed over the chains) and ratios (of the fleet's integer totals)
SWEEP_TOTALS = (("import_wh", "energy_wh_import"), ("export_wh", "energy_wh_export"), ("charge_wh", "energy_wh_charge"),
                ("discharge_wh", "energy_wh_discharge"), ("loss_wh", "energy_wh_loss"))
SWEEP_RATIOS = ("self_consumption", "self_sufficiency", "full_cycles")

DISPATCH_SWEEP_OPTIONS = SWEEP_OPTIONS + ("charge_above_w", "discharge_above_w", "feed_in_limit_w")
# the dispatch-sweep CSV: a row per variant -- its parameters (feed_in_limit_w `none` without a limit), then (header,
# key of dispatch.sweep_summary) fleet totals, the largest peaks of any chain (W) and ratios
DISPATCH_SWEEP_TOTALS = SWEEP_TOTALS + (("curtailed_wh", "energy_wh_curtailed"), ("peak_import_w", "peak_w_import"),
                                        ("peak_export_w", "peak_w_export"))
DISPATCH_SWEEP_RATIOS = SWEEP_RATIOS + ("curtailed_share",)

# per sweep command: the BatchedSim method that enables its table and the attribute with the quantized parameters, the
# module whose sweep_summary(fleet=True) gives the CSV's rows, and the CSV's columns
SWEEPS = {
    "battery-sweep": dict(enable="enable_battery_sweep", params="battery_params", module="battery",
                          options=SWEEP_OPTIONS, totals=SWEEP_TOTALS, ratios=SWEEP_RATIOS),
    "dispatch-sweep": dict(enable="enable_dispatch_sweep", params="dispatch_params", module="dispatch",
                           options=DISPATCH_SWEEP_OPTIONS, totals=DISPATCH_SWEEP_TOTALS, ratios=DISPATCH_SWEEP_RATIOS),
}


def _variant_lists(command, lists):
    k = max(len(v) for v in lists.values())
    bad = [name for name, v in lists.items() if len(v) not in (1, k)]
    if bad:
        raise click.ClickException(f"{command}: --{bad[0].replace('_', '-')} has {len(lists[bad[0]])} values; every list "
                                   f"needs one length ({k} here) or length 1: a list is one value per variant")
    return k, {name: list(v) * (k if len(v) == 1 else 1) for name, v in lists.items()}


def sweep_lists(**lists):
    """The battery-sweep options (lists of floats) as one value per variant: every list has the one length K or
    length 1 (repeated); click.ClickException otherwise.  Returns (K, {option: [K floats]})."""
    return _variant_lists("battery-sweep", lists)


def dispatch_sweep_lists(**lists):
    """The dispatch-sweep options likewise (lists of floats; --feed-in-limit-w's entries may be None: no limit)."""
    return _variant_lists("dispatch-sweep", lists)


def _fleet_rows(command, raw, interval_s, params):
    from importlib import import_module
    fleet = import_module("." + SWEEPS[command]["module"], __package__).sweep_summary(raw, interval_s, params, fleet=True)
    return [{k: float(v[i]) for k, v in fleet.items()} for i in range(len(raw))]


def sweep_fleet_rows(raw, interval_s, params):
    """A dict per variant of the fleet's totals (SWEEP_TOTALS, Wh over all the chains) and ratios (SWEEP_RATIOS, of
    the fleet's integer sums) from a raw sweep table [K, n_iv, 10, n]: battery.sweep_summary(fleet=True)."""
    return _fleet_rows("battery-sweep", raw, interval_s, params)


def dispatch_sweep_fleet_rows(raw, interval_s, params):
    """A dict per variant of the fleet's totals and ratios (DISPATCH_SWEEP_TOTALS, DISPATCH_SWEEP_RATIOS) from a raw
    dispatch sweep table [K, n_iv, 13, n]: dispatch.sweep_summary(fleet=True)."""
    return _fleet_rows("dispatch-sweep", raw, interval_s, params)


def _sweep_command(command, file, batch, start, seconds, seed, interval_s, all_chains, lists):
    """The `battery-sweep` and `dispatch-sweep` commands (SWEEPS): a row per variant to FILE, every variant's raw table
    to the .npz.  lists: a list per option of the command, in any order."""
    sweep = SWEEPS[command]
    k, opts = _variant_lists(command, {o: lists[o] for o in sweep["options"]})
    sim = _open_sim(batch, start, seconds, seed, "fp64")
    import torch
    with _refusals():   # (also too many variants: the module's quantize_sweep_params)
        raw = getattr(sim, sweep["enable"])(int(seconds), int(interval_s), n_variants=k, **opts)
    sim.run(int(seconds), trace=())
    torch.cuda.synchronize()
    raw, params = raw.cpu().numpy(), getattr(sim, sweep["params"]).cpu().numpy()
    _warn_faulted(sim, batch, "their tables hold the seconds before the fault")
    rows = _fleet_rows(command, raw, interval_s, params)
    cell = lambda x: "none" if x is None else repr(float(x))   # (a feed-in limit)
    with open(file, "w") as f:
        f.write(",".join(("variant",) + sweep["options"] + tuple(h for h, _ in sweep["totals"]) + sweep["ratios"]) + "\n")
        for v, row in enumerate(rows):
            f.write(",".join([str(v)] + [cell(opts[o][v]) for o in sweep["options"]]
                             + [repr(row[key]) for _, key in sweep["totals"]]
                             + [repr(row[key]) for key in sweep["ratios"]]) + "\n")
    if all_chains:
        import numpy as np
        np.savez(all_chains, raw=raw, params=params, soc=sim.soc.cpu().numpy(), interval_s=interval_s)
    click.echo(f"wrote {k} rows to {file}" + (f" and {k} x {batch} chains to {all_chains}" if all_chains else ""))


@main.command("battery-sweep")
@click.argument("file")
@common
@table_options(precision=False, every="variant's raw table of every chain")
@battery_options("one value per variant")
def battery_sweep(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, interval_s, all_chains, **lists):
    """Every chain behind each of K candidate batteries in one fp64 engine run: a CSV row per variant to FILE."""
    _batch_mode(verbose, realtime, batch, "battery-sweep")
    _sweep_command("battery-sweep", file, batch, start, seconds, seed, interval_s, all_chains, lists)


@main.command("dispatch-sweep")
@click.argument("file")
@common
@table_options(precision=False, every="variant's raw table of every chain")
@battery_options("one value per variant")
@dispatch_options
def dispatch_sweep(file, amqp_url, exchange, verbose, realtime, batch, start, seconds, seed, interval_s, all_chains, **lists):
    """Every chain under each of K dispatch rules (battery, thresholds, feed-in limit) in one fp64 engine run: a CSV
    row per variant to FILE."""
    _batch_mode(verbose, realtime, batch, "dispatch-sweep")
    _sweep_command("dispatch-sweep", file, batch, start, seconds, seed, interval_s, all_chains, lists)


if __name__ == "__main__":
    main()

