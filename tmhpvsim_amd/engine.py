"""Batched simulator: N chains (site x scenario) advanced on one MI355X.

PyTorch-ROCm is used only for device memory and the stream; all compute runs
in libtmhpvsim.so (HIP, gfx950) through the C-ABI of include/tmhpvsim.h.
Chain state is a structure-of-arrays buffer owned by this object; traces are
time-major [step, chain] tensors; statistics are accumulated on the GPU.
"""
from __future__ import annotations

import ctypes as C
import importlib

import numpy as np

from . import _lib
from .clock import make_clock
from .params import ModelParams, RNG_INJECTED

TRACE_FIELDS = ("csi", "covered", "pv", "meter", "residual")
ROLL_MAX = 731 * 86400   # steps per rolling clock (<= 6 DST changes in two years)
DEFAULT_HIST = dict(n_bins=4096, lo=-300.0, hi=9000.0)


def _torch():
    import torch
    return torch


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# The interval tables (tmh_intervals and its typedefs): per-chain cells per metering interval, one kind
# per sim.  Per kind: its module (COLUMNS, to_watts; the C setter is tmh_set_<kind>), the noun of its
# messages, and what it refuses beside it -- at enable_<kind> (attribute, message) and in run() (its name
# beside a fleet series, the other kinds with their message, the message of a run with traces).  The sim
# keeps kind's raw tensor in <kind>_raw and its descriptor in _<kind>.
_TABLES = {
    "intervals": dict(
        noun="intervals", name="interval metering",
        enable_excludes=(
            ("_registers", "the import / export registers are enabled: their table holds the intervals' columns "
                           "(registers.to_intervals); one of the two per sim"),
            ("_demand", "the demand registers are enabled: their table holds the intervals' columns; one of the two per sim")),
        run_excludes=(),
        no_trace="an interval-metering run takes no traces (trace=()): sum the traces instead (intervals.from_traces)"),
    "registers": dict(
        noun="registers", name="the registers",
        enable_excludes=(
            ("_intervals", "interval metering is enabled: the registers table holds the intervals' columns "
                           "(registers.to_intervals); one of the two per sim"),
            ("_demand", "the demand registers are enabled: their table holds the registers' columns "
                        "(demand.to_registers); one of the two per sim")),
        run_excludes=(("_intervals",), "the registers and interval metering are both enabled: one of the two per sim"),
        no_trace="a registers run takes no traces (trace=()): sum the traces instead (registers.from_traces)"),
    "demand": dict(
        noun="demand registers", name="the demand registers",
        enable_excludes=tuple(
            (attr, f"{what} is enabled: one table output per sim (the demand table holds the registers' "
                   "and the intervals' columns, demand.to_registers)")
            for attr, what in (("_series", "a fleet series"), ("_intervals", "interval metering"),
                               ("_registers", "the import / export registers"))),
        run_excludes=(("_intervals", "_registers"), "the demand registers and interval metering or the import / export "
                                                    "registers are both enabled: one of them per sim"),
        no_trace="a demand run takes no traces (trace=()): take the peaks of the traces instead (demand.from_traces)"),
    # battery storage (enable_storage: the battery's arguments beside the table's; fp64 sims only)
    "storage": dict(
        noun="storage tables", name="battery storage",
        enable_excludes=tuple(
            (attr, f"{what} is enabled: one table output per sim (battery storage runs alone)")
            for attr, what in (("_series", "a fleet series"), ("_intervals", "interval metering"),
                               ("_registers", "the import / export registers"), ("_demand", "the demand registers"))),
        run_excludes=(("_intervals", "_registers", "_demand"), "battery storage and another interval table are both "
                                                               "enabled: one of them per sim"),
        no_trace="a storage run takes no traces (trace=()): run the battery over the traces instead (storage.from_traces)"),
    # the battery kind (enable_battery: storage with losses and per-chain parameters; fp64 sims only)
    "battery": dict(
        noun="battery tables", name="the battery kind",
        enable_excludes=tuple(
            (attr, f"{what} is enabled: one table output per sim (the battery kind runs alone)")
            for attr, what in (("_series", "a fleet series"), ("_intervals", "interval metering"),
                               ("_registers", "the import / export registers"), ("_demand", "the demand registers"))),
        run_excludes=(("_intervals", "_registers", "_demand", "_storage"), "the battery kind and another interval table "
                                                                           "are both enabled: one of them per sim"),
        no_trace="a battery run takes no traces (trace=()): run the battery over the traces instead (battery.from_traces)"),
    # battery dispatch (enable_dispatch: the battery kind with thresholds and a feed-in limit; fp64 sims only)
    "dispatch": dict(
        noun="dispatch tables", name="battery dispatch",
        enable_excludes=tuple(
            (attr, f"{what} is enabled: one table output per sim (battery dispatch runs alone)")
            for attr, what in (("_series", "a fleet series"), ("_intervals", "interval metering"),
                               ("_registers", "the import / export registers"), ("_demand", "the demand registers"),
                               ("_battery_fleet", "a battery fleet series"))),
        run_excludes=(("_intervals", "_registers", "_demand", "_storage", "_battery"),
                      "battery dispatch and another interval table are both enabled: one of them per sim"),
        no_trace="a dispatch run takes no traces (trace=()): run the battery over the traces instead (dispatch.from_traces)"),
    # scheduled dispatch (enable_schedule: battery dispatch with a rule per metering interval and grid charging; fp64
    # sims, one site)
    "schedule": dict(
        noun="schedule tables", name="the schedule",
        enable_excludes=tuple(
            (attr, f"{what} is enabled: one table output per sim (the schedule runs alone)")
            for attr, what in (("_series", "a fleet series"), ("_intervals", "interval metering"),
                               ("_registers", "the import / export registers"), ("_demand", "the demand registers"),
                               ("_battery_fleet", "a battery fleet series"))),
        run_excludes=(("_intervals", "_registers", "_demand", "_storage", "_battery", "_dispatch"),
                      "the schedule and another interval table are both enabled: one of them per sim"),
        no_trace="a schedule run takes no traces (trace=()): run the battery over the traces instead (schedule.from_traces)"),
}
for _kind, _t in _TABLES.items():   # no table beside battery storage, whichever was enabled first
    if _kind != "storage":
        _t["enable_excludes"] += (("_storage", "battery storage is enabled: one table output per sim "
                                               "(battery storage runs alone)"),)
    if _kind != "battery":
        _t["enable_excludes"] += (("_battery", "the battery kind is enabled: one table output per sim "
                                               "(the battery kind runs alone)"),)
    if _kind != "dispatch":
        _t["enable_excludes"] += (("_dispatch", "battery dispatch is enabled: one table output per sim "
                                                "(battery dispatch runs alone)"),)
    # (enable_battery_sweep: the battery sweep, a kind with descriptor and attributes of its own)
    _t["enable_excludes"] += (("_battery_sweep", "the battery sweep is enabled: one table output per sim "
                                                 "(the battery sweep runs alone)"),)
    # (enable_dispatch_sweep: the dispatch sweep, likewise)
    _t["enable_excludes"] += (("_dispatch_sweep", "the dispatch sweep is enabled: one table output per sim "
                                                  "(the dispatch sweep runs alone)"),)
    # (enable_schedule: the last kind, so that everything refused before it is refused in the same words)
    if _kind != "schedule":
        _t["enable_excludes"] += (("_schedule", "the schedule is enabled: one table output per sim "
                                                "(the schedule runs alone)"),)
    # (enable_schedule_sweep: the schedule sweep, as the two sweeps above; the last words of every kind's list)
    _t["enable_excludes"] += (("_schedule_sweep", "the schedule sweep is enabled: one table output per sim "
                                                  "(the schedule sweep runs alone)"),)
# the sweeps: a table per variant; what they refuse beside them at enable_<kind> is _enable_battery's to say
_TABLES["battery_sweep"] = dict(
    noun="battery sweep tables", name="the battery sweep", enable_excludes=(), run_excludes=(),
    no_trace="a battery sweep run takes no traces (trace=()): run the batteries over the traces instead "
             "(battery.sweep_from_traces)")
_TABLES["dispatch_sweep"] = dict(
    noun="dispatch sweep tables", name="the dispatch sweep", enable_excludes=(), run_excludes=(),
    no_trace="a dispatch sweep run takes no traces (trace=()): run the rules over the traces instead "
             "(dispatch.sweep_from_traces)")
_TABLES["schedule_sweep"] = dict(
    noun="schedule sweep tables", name="the schedule sweep", enable_excludes=(), run_excludes=(),
    no_trace="a schedule sweep run takes no traces (trace=()): run the variants over the traces instead "
             "(schedule.sweep_from_traces)")

# The battery family: the kinds of _TABLES that carry a state of charge per chain (`sim.soc`) through a work buffer,
# one of them per sim, through one enabler (_enable_battery), one setter (_set_battery) and one work buffer
# (_work_window).  Per kind: its module; its parameter rows per variant (0: storage's three integers, None: the
# schedule's 6 + 4 R); its ctypes struct (the C setter is tmh_set_<kind>); whether it has variants; whether per-chain
# sites are refused; how enable_<kind> checks the window ("long": n_steps and interval_s, "short": interval_s <=
# MAX_INTERVAL_S, None: the kind's own arguments do); the attribute its parameters are published in; the attribute
# that keeps its descriptor.
_BATTERIES = {
    "storage": dict(mod="storage", rows=0, cls=_lib.Storage, variants=False, one_site=False, window=None,
                    params=None, desc="_storage_desc"),
    "battery": dict(mod="battery", rows=6, cls=_lib.Battery, variants=False, one_site=False, window="short",
                    params="battery_params", desc="_battery_desc"),
    "dispatch": dict(mod="dispatch", rows=9, cls=_lib.Dispatch, variants=False, one_site=False, window="short",
                     params="dispatch_params", desc="_dispatch_desc"),
    "schedule": dict(mod="schedule", rows=None, cls=_lib.Schedule, variants=False, one_site=True, window="long",
                     params="schedule_params", desc="_schedule_desc"),
    "battery_sweep": dict(mod="battery", rows=6, cls=_lib.BatterySweep, variants=True, one_site=True, window="long",
                          params="battery_params", desc="_sweep_desc"),
    "dispatch_sweep": dict(mod="dispatch", rows=9, cls=_lib.DispatchSweep, variants=True, one_site=True, window="long",
                           params="dispatch_params", desc="_dsweep_desc"),
    "schedule_sweep": dict(mod="schedule", rows=None, cls=_lib.ScheduleSweep, variants=True, one_site=True, window="long",
                           params="schedule_sweep_params", desc="_ssweep_desc"),
}


class BatchedSim:
    """Advance chains [chain0, chain0 + n_chains) second by second.

    Parameters
    ----------
    n_chains : chains on this device (each is one ClearskyindexModel + PVModel
        + meter, tmhpvsim/clearskyindexmodel.py:44, pvmodel.py:11, metersim.py:49)
    start : constructor time of every chain (datetime / str); step 0 = next(start)
    tz : None (naive wall clock) or a zone name ("Europe/Berlin", as pvmodel.py:19)
    params : tmhpvsim_amd.params.ModelParams (modes, seed, shape table, site, PV system)
    precision : "fp32" (per-second CSI/PV math in fp32; Markov state fp64) or "fp64"
    chain0 : global id of the first chain (keyed RNG -> partition-independent results)
    injected : optional device tensor [n_chains, L] of uniforms (RNG_INJECTED mode)
    horizon : steps covered by one wall clock (its DST table holds 8 changes); a run
        past it installs the next rolling clock (tmh_set_clock), so runs are unbounded
    shape_tables : optional per-chain hourly cloud-cover tables (shapes [n, 6, 4],
        is_t [n, 6]; e.g. params.site_shape_tables) in place of params.shapes —
        one table per site of a lat/lon sweep (tmh_set_shape_tables)
    sites : optional per-chain PV sites [n, 8] in Site.as_array() order (e.g.
        params.site_grid), or (sites, linke [n, 12]); columns 0-5 vary per chain,
        temp_air and wind stay params.site's (tmh_set_sites)
    """

    def __init__(self, n_chains, start, tz=None, params: ModelParams | None = None, precision="fp32",
                 chain0=0, device=None, injected=None, horizon=400 * 86400, kernel_path="auto",
                 shape_tables=None, sites=None):
        torch = _torch()
        L = _lib.load()
        self.L = L
        self.params = params or ModelParams()
        self.n = int(n_chains)
        self.chain0 = int(chain0)
        self.precision = _lib.TMH_FP64 if precision in ("fp64", "f64", 64) else _lib.TMH_FP32
        self.real = torch.float64 if self.precision == _lib.TMH_FP64 else torch.float32
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError("BatchedSim runs on a GPU device (there is no CPU path)")
        self.horizon = int(horizon)
        self._start, self._tz = start, tz
        self.clock = make_clock(start, self.horizon, tz)
        kp = {"auto": _lib.PATH_AUTO, "sequential": _lib.PATH_SEQUENTIAL,
              "time_parallel": _lib.PATH_TIME_PARALLEL}[kernel_path]
        P = _lib.make_params(self.params, self.precision, kp)
        ck = self.clock.as_struct()
        eng = C.c_void_p()
        _lib.check(L.tmh_engine_create(C.byref(P), C.byref(ck), self.device.index or 0, C.byref(eng)))
        self._eng = eng
        self.path = {1: "sequential", 2: "time_parallel"}[L.tmh_engine_path(eng)]
        self.state = torch.zeros(L.tmh_state_bytes(self.n), dtype=torch.uint8, device=self.device)
        self._offsets = _lib.state_offsets(self.n)
        self.injected = None
        self._us = None
        if self.params.rng_mode == RNG_INJECTED:
            if injected is None:
                raise ValueError("RNG_INJECTED mode needs `injected` uniforms [n_chains, L]")
            inj = torch.as_tensor(injected, dtype=torch.float64, device=self.device).contiguous()
            if inj.shape[0] != self.n:
                raise ValueError("injected must have one row per chain")
            self.injected = inj
            self._us = _lib.UStream(inj.data_ptr(), inj.shape[1], inj.shape[1])
        self.tables = None
        if shape_tables is not None:
            sh, it = shape_tables if isinstance(shape_tables, tuple) else (shape_tables, None)
            sh = torch.as_tensor(np.asarray(sh, dtype=np.float64) if not torch.is_tensor(sh) else sh,
                                 dtype=torch.float64, device=self.device).contiguous()
            if tuple(sh.shape) != (self.n, 6, 4):
                raise ValueError(f"shape_tables must be [n_chains, 6, 4], got {tuple(sh.shape)}")
            if it is not None:
                it = torch.as_tensor(np.asarray(it) if not torch.is_tensor(it) else it,
                                     dtype=torch.int32, device=self.device).contiguous()
                if tuple(it.shape) != (self.n, 6):
                    raise ValueError(f"shape_tables is_t must be [n_chains, 6], got {tuple(it.shape)}")
            self.tables = (sh, it)   # the engine reads them on every launch: keep them alive
            _lib.check(L.tmh_set_shape_tables(self._eng, _ptr(sh), _ptr(it) if it is not None else None, self.n))
        self.sites = None
        if sites is not None:
            si, li = sites if isinstance(sites, tuple) else (sites, None)
            si = torch.as_tensor(np.asarray(si, dtype=np.float64) if not torch.is_tensor(si) else si,
                                 dtype=torch.float64, device=self.device).contiguous()
            if tuple(si.shape) != (self.n, 8):
                raise ValueError(f"sites must be [n_chains, 8], got {tuple(si.shape)}")
            if li is not None:
                li = torch.as_tensor(np.asarray(li, dtype=np.float64) if not torch.is_tensor(li) else li,
                                     dtype=torch.float64, device=self.device).contiguous()
                if tuple(li.shape) != (self.n, 12):
                    raise ValueError(f"sites linke must be [n_chains, 12], got {tuple(li.shape)}")
            self.sites = (si, li)
            _lib.check(L.tmh_set_sites(self._eng, _ptr(si), _ptr(li) if li is not None else None, self.n))
        self.step = 0
        self.hist = None
        self.chain_acc = None
        self._hist_spec = None
        self.series_raw = None    # int64 [n_groups, n_steps, 4] (enable_series)
        self._series = None
        for kind in _TABLES:   # <kind>_raw: int64 [n_intervals, cols, n] ([K, n_intervals, cols, n]: a sweep) (enable_<kind>)
            setattr(self, kind + "_raw", None)
            setattr(self, "_" + kind, None)
        # the battery family (_BATTERIES): soc int64 [n] ([K, n]: a sweep), the batteries' state of charge; the
        # parameters int64 [6, n] (enable_battery), [9, n] (enable_dispatch), [6 + 4 R, n] (enable_schedule) or
        # [K, 6 / 9, n] (the sweeps); schedule_rules uint8 [n_intervals]: the rule of each of the table's intervals
        self.soc = self.battery_params = self.dispatch_params = self.schedule_params = self.schedule_rules = None
        # the schedule sweep's parameters int64 [K, 6 + 4 R, n] and rule arrays uint8 [K, n_intervals]
        self.schedule_sweep_params = self.schedule_sweep_rules = None
        self._battery_args = self._battery_work = None   # (soc, params, the struct's last fields), the work buffer
        for t in _BATTERIES.values():
            setattr(self, t["desc"], None)
        self.battery_fleet_raw = None   # int64 [n_groups, n_steps, 8]: the battery fleet series (enable_battery_fleet)
        self._battery_fleet = None
        self.dispatch_fleet_raw = None   # int64 [n_groups, n_steps, 9]: the dispatch fleet series (enable_dispatch_fleet)
        self._dispatch_fleet = None
        self.compact_slots = []      # slots each window of the last compact=True run ran on (run())
        self._last_scratch = None
        with torch.cuda.device(self.device):
            _lib.check(L.tmh_init(self._eng, _ptr(self.state), self.chain0, self.n,
                                  C.byref(self._us) if self._us is not None else None, self._stream()))

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def __del__(self):
        try:
            if getattr(self, "_eng", None):
                self.L.tmh_engine_destroy(self._eng)
                self._eng = None
        except Exception:
            pass

    # ------------------------------------------------------------------ state
    def state_field(self, name):
        """Device view of one SoA state field ([n], or [n, TMH_SIGMA_CAP] for the sigma arrays)."""
        torch = _torch()
        i = _lib.STATE_FIELDS.index(name)
        dt = {np.float64: torch.float64, np.int32: torch.int32, np.uint32: torch.int32,
              np.float32: torch.float32}[_lib.STATE_DTYPES[name]]
        esz = 8 if dt == torch.float64 else 4
        rows = _lib.TMH_SIGMA_CAP if name.startswith("sigma_c") else (2 if name.startswith("fn_") else 1)
        o = int(self._offsets[i])
        v = self.state[o:o + esz * self.n * rows].view(dt)
        return v.view(self.n, rows) if rows > 1 else v

    def status(self):
        return self.state_field("status").cpu().numpy().astype(np.uint32)

    # ------------------------------------------------------------------ stats
    def enable_stats(self, n_bins=4096, lo=-300.0, hi=9000.0, histogram=True):
        torch = _torch()
        self._hist_spec = (int(n_bins), float(lo), float(hi), bool(histogram))
        self.hist = torch.zeros(int(n_bins), dtype=torch.int64, device=self.device) if histogram else None
        self.chain_acc = torch.zeros(4, self.n, dtype=torch.float64, device=self.device)
        self.chain_acc[3].fill_(-float("inf"))

    def _stats_struct(self):
        if self.chain_acc is None:
            return None
        n_bins, lo, hi, _ = self._hist_spec
        return _lib.Stats(self.hist.data_ptr() if self.hist is not None else None, n_bins, 0, lo, hi,
                          self.chain_acc.data_ptr())

    # ------------------------------------------------------------------ fleet series
    def enable_series(self, n_steps, step0=None, group_chains=0, buffer=None):
        """Accumulate the fleet series (tmhpvsim_amd.series: exact per-second integer sums
        of pv and meter, n_ok and the covered count over the chains) of steps [step0,
        step0 + n_steps) in every later run; step0 defaults to the current step.  Chain i
        belongs to group i // group_chains (0: one group; else a multiple of 512).
        buffer: an int64 device tensor [n_groups, n_steps, 4] to add into (several sims
        sharing one series); by default a zeroed one.  Runs with a series take no traces
        (trace=()) and no compaction; n_steps=None switches the series off."""
        torch = _torch()
        if n_steps is None:
            _lib.check(self.L.tmh_set_series(self._eng, None))
            self.series_raw, self._series = None, None
            return None
        n_steps, gc = int(n_steps), int(group_chains)
        if n_steps < 1 or gc < 0 or gc % 512:
            raise ValueError("enable_series: n_steps >= 1, group_chains 0 or a multiple of 512")
        n_groups = 1 if gc == 0 else -(-self.n // gc)
        if buffer is None:
            buffer = torch.zeros(n_groups, n_steps, 4, dtype=torch.int64, device=self.device)
        elif (buffer.dtype != torch.int64 or buffer.device != self.device or not buffer.is_contiguous()
              or buffer.dim() != 3 or buffer.shape[0] < n_groups or tuple(buffer.shape[1:]) != (n_steps, 4)):
            raise ValueError(f"series buffer must be a contiguous int64 [>= {n_groups}, {n_steps}, 4] tensor on {self.device}")
        st = _lib.Series(buffer.data_ptr(), self.step if step0 is None else int(step0), n_steps, gc,
                         int(buffer.shape[0]), 0)
        _lib.check(self.L.tmh_set_series(self._eng, C.byref(st)))
        self.series_raw, self._series = buffer, st
        return buffer

    def series(self, bin_s=1, mean=False):
        """The series in watts (series.to_watts of series_raw): pv, meter, residual, n_ok and
        the covered fraction per bin of bin_s seconds, [n_groups, n_bins] each."""
        from .series import to_watts
        if self.series_raw is None:
            raise ValueError("no series: call enable_series first")
        _torch().cuda.synchronize(self.device)
        return to_watts(self.series_raw, bin_s=bin_s, mean=mean)

    # ------------------------------------------------------------------ interval tables
    def _enable_table(self, kind, n_steps, interval_s, step0, buffer):
        """enable_intervals, enable_registers and enable_demand (_TABLES[kind])."""
        torch = _torch()
        if kind in _BATTERIES:   # (its descriptor holds the table's: _set_battery)
            setter = lambda eng, st: self._set_battery(kind, st._obj if st is not None else None)
        else:
            setter = getattr(self.L, "tmh_set_" + kind)
        if n_steps is None:
            _lib.check(setter(self._eng, None))
            setattr(self, kind + "_raw", None)
            setattr(self, "_" + kind, None)
            return None
        for attr, message in _TABLES[kind]["enable_excludes"]:
            if getattr(self, attr) is not None:
                raise ValueError(message)
        mod = importlib.import_module("." + kind, __package__)
        n_steps, interval_s, nc = int(n_steps), int(interval_s), len(mod.COLUMNS)
        if n_steps < 1 or interval_s < 1:
            raise ValueError(f"enable_{kind}: n_steps >= 1 and interval_s >= 1")
        nk = mod.n_intervals(n_steps, interval_s)
        if buffer is None:
            buffer = torch.zeros(nk, nc, self.n, dtype=torch.int64, device=self.device)
        elif (buffer.dtype != torch.int64 or buffer.device != self.device or tuple(buffer.shape) != (nk, nc, self.n)):
            raise ValueError(f"{kind} buffer must be an int64 [{nk}, {nc}, {self.n}] tensor on {self.device}")
        ld = int(buffer.stride(1))
        if ld < self.n or (self.n > 1 and buffer.stride(2) != 1) or (nk > 1 and buffer.stride(0) != nc * ld):
            raise ValueError(f"{kind} buffer strides {tuple(buffer.stride())}: need ({nc} ld, ld, 1) with ld >= {self.n}")
        st = _lib.Intervals(buffer.data_ptr(), self.step if step0 is None else int(step0), n_steps, interval_s, ld)
        _lib.check(setter(self._eng, C.byref(st)))
        setattr(self, kind + "_raw", buffer)
        setattr(self, "_" + kind, st)
        return buffer

    def _table_watts(self, kind):
        """intervals(), registers() and demand(): <kind>.to_watts of the raw table."""
        raw, st = getattr(self, kind + "_raw"), getattr(self, "_" + kind)
        if raw is None:
            raise ValueError(f"no {_TABLES[kind]['noun']}: call enable_{kind} first")
        _torch().cuda.synchronize(self.device)
        return importlib.import_module("." + kind, __package__).to_watts(raw, st.interval_s, n_steps=st.n_steps)

    # ------------------------------------------------------------------ interval metering
    def enable_intervals(self, n_steps, interval_s=900, step0=None, buffer=None):
        """Accumulate every chain's interval meter (tmhpvsim_amd.intervals: exact per-chain
        integer sums of pv and meter, the ok seconds and the covered seconds per metering
        interval of interval_s seconds) over steps [step0, step0 + n_steps) in every later
        run; step0 defaults to the current step.  Returns the raw int64 tensor
        [n_intervals, 4, n].  buffer: an int64 device tensor of that shape to add into; it may
        be a view with strides (4 ld, ld, 1) -- a column slice big[:, :, a:b] of a contiguous
        table, so several batches or shards fill one table (ld is read from the strides); by
        default a zeroed one.  Runs with intervals take no traces (trace=()) and no fleet
        series; compaction is allowed.  n_steps=None switches the output off."""
        return self._enable_table("intervals", n_steps, interval_s, step0, buffer)

    def intervals(self):
        """The interval table in watts and watt-hours (intervals.to_watts of intervals_raw):
        pv, meter, residual (means over the ok seconds), energy_wh_*, n_ok and the covered
        fraction, [n_intervals, n] each."""
        return self._table_watts("intervals")

    # ------------------------------------------------------------------ import / export registers
    def enable_registers(self, n_steps, interval_s=900, step0=None, buffer=None):
        """Accumulate every chain's bidirectional meter (tmhpvsim_amd.registers: the interval
        meter's four columns plus the import and export registers -- the exact integer sums
        of max(meter - pv, 0) and max(pv - meter, 0) -- per metering interval of interval_s
        seconds) over steps [step0, step0 + n_steps) in every later run; step0 defaults to
        the current step.  Returns the raw int64 tensor [n_intervals, 6, n].  buffer: an int64
        device tensor of that shape to add into; it may be a view with strides (6 ld, ld, 1)
        -- a column slice big[:, :, a:b] of a contiguous table (ld is read from the strides);
        by default a zeroed one.  Runs with registers take no traces (trace=()), no fleet
        series and no interval metering beside them; compaction is allowed.  n_steps=None
        switches the output off."""
        return self._enable_table("registers", n_steps, interval_s, step0, buffer)

    def registers(self):
        """The registers table in watts and watt-hours (registers.to_watts of registers_raw): the
        intervals' keys plus energy_wh_import, energy_wh_export, energy_wh_self and the
        self_consumption and self_sufficiency ratios, [n_intervals, n] each."""
        return self._table_watts("registers")

    # ------------------------------------------------------------------ demand registers
    def enable_demand(self, n_steps, interval_s=900, step0=None, buffer=None):
        """Keep every chain's demand registers (tmhpvsim_amd.demand: the import / export
        registers' six columns plus the peak import and the peak export of each metering
        interval of interval_s seconds as packed keys -- the quantised power above the
        complement of the second's offset, combined by maximum, so the earliest second at the
        peak wins) over steps [step0, step0 + n_steps) in every later run; step0 defaults to
        the current step.  Returns the raw int64 tensor [n_intervals, 8, n].  buffer: an int64
        device tensor of that shape to accumulate into; it may be a view with strides
        (8 ld, ld, 1) -- a column slice big[:, :, a:b] of a contiguous table (ld is read from
        the strides); by default a zeroed one.  Runs with demand registers take no traces
        (trace=()), no fleet series, no interval metering and no import / export registers
        beside them (the table holds their columns); compaction is allowed.  n_steps=None
        switches the output off."""
        return self._enable_table("demand", n_steps, interval_s, step0, buffer)

    def demand(self):
        """The demand table in watts and watt-hours (demand.to_watts of demand_raw): the
        registers' keys plus peak_import, peak_export, t_peak_import, t_peak_export and
        load_factor, [n_intervals, n] each."""
        return self._table_watts("demand")

    # ------------------------------------------------------------------ the battery family
    def _enable_battery(self, kind, n_steps, interval_s, step0, buffer, soc, params, soc0_wh, quantize, n_variants=None,
                        last=lambda host: ()):
        """enable_storage, enable_battery, enable_dispatch, enable_schedule and the three sweeps (_BATTERIES[kind]).
        quantize(): the kind's quantities as host parameters, called when no params tensor is given (storage: its
        three integers and the starting state of charge); last(host): the fields of the kind's struct after params
        (the schedule's and the schedule sweep's rule array and rule count; a sweep's variant count follows them).  A refused call leaves what was enabled before as it was."""
        torch = _torch()
        t, name, label = _BATTERIES[kind], _TABLES[kind]["name"], kind.replace("_", " ")
        if n_steps is None:
            if kind in ("dispatch", "schedule") and getattr(self, "_" + kind) is not None and self._dispatch_fleet is not None:
                self.enable_dispatch_fleet(None)   # (the kind's own output: off with it)
            if getattr(self, "_" + kind) is not None:   # (else soc and the work buffer may be another kind's)
                self.soc = self._battery_work = self._battery_args = None
                setattr(self, t["desc"], None)
                for attr in (t["params"],) + (("schedule_rules",) if kind == "schedule" else
                                              ("schedule_sweep_rules",) if kind == "schedule_sweep" else ()):
                    if attr:
                        setattr(self, attr, None)
            return self._enable_table(kind, None, interval_s, step0, buffer)
        if self.precision != _lib.TMH_FP64:
            raise ValueError(f"{name} needs precision='fp64': an fp32 engine replaces its guard-band seconds "
                             "after the expansion, and the state of charge depends on every earlier second")
        if t["variants"]:
            if self._series is not None:
                raise ValueError(f"a fleet series is enabled: one table output per sim ({name} runs alone)")
            if self._battery_fleet is not None:
                raise ValueError(f"a battery fleet series is enabled: it is the battery kind's ({name} runs alone)")
            for other, ot in _TABLES.items():
                if other != kind and getattr(self, "_" + other) is not None:
                    raise ValueError(f"{ot['name']} is enabled: one table output per sim ({name} runs alone)")
        if t["one_site"] and self.sites is not None:
            raise ValueError(f"{name} cannot run with per-chain sites")
        mod = importlib.import_module("." + t["mod"], __package__)
        if t["window"] == "long" and (int(n_steps) < 1 or int(interval_s) < 1 or int(interval_s) > mod.MAX_INTERVAL_S):
            raise ValueError(f"enable_{kind}: n_steps >= 1 and 1 <= interval_s <= {mod.MAX_INTERVAL_S}")
        if t["window"] == "short" and int(interval_s) > mod.MAX_INTERVAL_S:
            raise ValueError(f"enable_{kind}: interval_s <= {mod.MAX_INTERVAL_S}")
        rows, lead = t["rows"], "K, " if t["variants"] else ""
        if rows == 0:
            host, (*tail, x0) = None, quantize()
        elif params is None:
            host = quantize()
            params = torch.from_numpy(host).to(self.device)
        else:
            if (params.dtype != torch.int64 or params.device != self.device or params.dim() != (3 if t["variants"] else 2)
                    or params.shape[-1] != self.n or (rows is not None and params.shape[-2] != rows)
                    or (self.n > 1 and params.stride(-1) != 1)):
                raise ValueError(f"{label} params must be an int64 [{lead}{'6 + 4 R' if rows is None else rows}, {self.n}] "
                                 f"tensor on {self.device}, chains contiguous")
            host = getattr(mod, "check_sweep_params" if t["variants"] else "check_params")(params)
        if t["variants"]:
            K = int(host.shape[0])
            if n_variants is not None and int(n_variants) != K:
                raise ValueError(f"enable_{kind}: n_variants {n_variants} but parameters of {K} variants")
            tail, shape = tuple(last(host)) + (K,), (K, self.n)   # (the variant count: the struct's last field)
        else:
            if rows != 0:
                tail = last(host)
            shape = (self.n,)
        if soc is None:
            soc = (torch.full(shape, x0, dtype=torch.int64, device=self.device) if rows == 0 else
                   torch.from_numpy(mod.quantize_sweep_soc(soc0_wh, host) if t["variants"]
                                    else mod.quantize_soc(soc0_wh, host[:6])).to(self.device))
        elif (soc.dtype != torch.int64 or soc.device != self.device or tuple(soc.shape) != shape
              or (self.n > 1 and soc.stride(-1) != 1)):
            raise ValueError(f"{label} soc must be an int64 [{K}, {self.n}] tensor on {self.device}, chains contiguous"
                             if t["variants"] else
                             f"{label} soc must be a contiguous int64 [{self.n}] tensor on {self.device}")
        kept = self._battery_args
        self._battery_args = (soc, params, tuple(tail))
        try:
            if t["variants"]:
                raw = self._enable_sweep_table(kind, int(n_steps), int(interval_s), step0, buffer, len(mod.COLUMNS))
            else:
                raw = self._enable_table(kind, n_steps, interval_s, step0, buffer)
        except Exception:   # (refused: what was enabled before stays as it was)
            self._battery_args = kept
            raise
        self.soc = soc
        if t["params"]:
            setattr(self, t["params"], params)
        return raw

    def _enable_sweep_table(self, kind, n_steps, interval_s, step0, buffer, nc):
        """_enable_table for the sweeps: a table per variant, [K, n_intervals, nc, n], and the variants' parameters and
        state of charge (_battery_args) at the table's ld."""
        torch = _torch()
        label, (soc, params, (*_, K)) = kind.replace("_", " "), self._battery_args
        npar, nk = int(params.shape[1]), -(-n_steps // interval_s)
        if buffer is None:
            buffer = torch.zeros(K, nk, nc, self.n, dtype=torch.int64, device=self.device)
        elif buffer.dtype != torch.int64 or buffer.device != self.device or tuple(buffer.shape) != (K, nk, nc, self.n):
            raise ValueError(f"{label} buffer must be an int64 [{K}, {nk}, {nc}, {self.n}] tensor on {self.device}")
        ld = int(buffer.stride(2))
        if (ld < self.n or (self.n > 1 and buffer.stride(3) != 1) or (nk > 1 and buffer.stride(1) != nc * ld)
                or (K > 1 and buffer.stride(0) != nk * nc * ld)):
            raise ValueError(f"{label} buffer strides {tuple(buffer.stride())}: need ({nk * nc} ld, {nc} ld, ld, 1) "
                             f"with ld >= {self.n}")
        if int(params.stride(1)) != ld or (K > 1 and (int(params.stride(0)) != npar * ld or int(soc.stride(0)) != ld)):
            raise ValueError(f"{label} params strides {tuple(params.stride())}, soc strides {tuple(soc.stride())}: need "
                             f"({npar} ld, ld, 1) and (ld, 1) with the table's ld {ld}: slice them from tensors of the same width")
        table = _lib.Intervals(buffer.data_ptr(), self.step if step0 is None else int(step0), n_steps, interval_s, ld)
        _lib.check(self._set_battery(kind, table))
        setattr(self, kind + "_raw", buffer)
        setattr(self, "_" + kind, table)
        return buffer

    def _set_battery(self, kind, table):
        """tmh_set_<kind> of a battery-family kind with the table descriptor `table` (or None) and _battery_args.  The
        work buffer is sized for the default window of a run and grown by run() when a window needs more
        (_work_window).  The parameters' row stride must be the table's ld (one ld for both)."""
        t, setter = _BATTERIES[kind], getattr(self.L, "tmh_set_" + kind)
        if table is None:
            return setter(self._eng, None)
        torch = _torch()
        soc, params, tail = self._battery_args
        K = tail[-1] if t["variants"] else 1
        if params is not None and not t["variants"] and int(params.stride(0)) != int(table.ld):
            raise ValueError(f"{kind} params row stride {int(params.stride(0))} != the table's ld {int(table.ld)}: "
                             "slice both from tensors of the same width")
        nb = self.L.tmh_battery_sweep_work_bytes(self.n, min(int(table.n_steps), 86400), K)
        work = self._battery_work   # (kept from enable to enable; a sweep enabled again with more variants: the setter's floor)
        if work is None or (t["variants"] and work.numel() < nb):
            work = torch.empty(max(nb, 8), dtype=torch.uint8, device=self.device)
        st = t["cls"](table, soc.data_ptr(), work.data_ptr(), work.numel(), *(() if params is None else (params.data_ptr(),)),
                      *(x.data_ptr() if torch.is_tensor(x) else x for x in tail))
        rc = setter(self._eng, C.byref(st))
        if rc == 0:
            self._battery_work = work
            setattr(self, t["desc"], st)
        return rc

    def _work_window(self, win):
        """run(): the enabled battery-family kind's work buffer holds a window of `win` steps (a larger one replaces
        it, and the descriptor is set again)."""
        for kind, t in _BATTERIES.items():
            table = getattr(self, "_" + kind)
            if table is None:
                continue
            K = self._battery_args[2][-1] if t["variants"] else 1
            need = self.L.tmh_battery_sweep_work_bytes(self.n, int(win), K)
            if self._battery_work.numel() < need:
                _torch().cuda.synchronize(self.device)   # (launches of earlier runs may still read the old one)
                self._battery_work = _torch().empty(need, dtype=torch_uint8(), device=self.device)
                _lib.check(self._set_battery(kind, table))

    # ------------------------------------------------------------------ battery storage
    def enable_storage(self, n_steps, interval_s=900, *, capacity_wh=None, charge_w=None, discharge_w=None, soc0_wh=0.0,
                       step0=None, buffer=None, soc=None):
        """Put a battery behind every chain's meter (tmhpvsim_amd.storage: greedy self-consumption,
        lossless, integers in the series' units) and keep, per metering interval of interval_s seconds
        over steps [step0, step0 + n_steps), the interval table's four columns, the import and export
        with the battery, what the battery took and gave, and the state of charge at the interval's end.
        capacity_wh, charge_w and discharge_w are the battery's capacity and power limits (uniform over
        the batch, quantised by storage.quantize_params); every chain starts at soc0_wh.  Returns the raw
        int64 tensor [n_intervals, 9, n]; `sim.soc` is the int64 state of charge [n], advanced by every
        window.  buffer: as enable_registers (strides (9 ld, ld, 1)); soc: an int64 device tensor [n] to
        carry instead of a new one (a slice of a larger one: several batches beside each other).  fp64
        sims only: an fp32 engine replaces guard-band seconds after the expansion, and the state of
        charge depends on every earlier second.  Runs with storage take no traces, no fleet series and no
        other table; compaction is allowed.  n_steps=None switches the output off."""
        def quantize():
            if capacity_wh is None or charge_w is None or discharge_w is None:
                raise ValueError("enable_storage: capacity_wh, charge_w and discharge_w are required")
            from . import storage
            q = storage.quantize_params(capacity_wh, charge_w, discharge_w, soc0_wh)
            if int(interval_s) > storage.MAX_INTERVAL_S:
                raise ValueError(f"enable_storage: interval_s <= {storage.MAX_INTERVAL_S}")
            return q
        return self._enable_battery("storage", n_steps, interval_s, step0, buffer, soc, None, soc0_wh, quantize)

    def storage(self):
        """The storage table in watts and watt-hours (storage.to_watts of storage_raw): the intervals'
        keys plus energy_wh_import, energy_wh_export, energy_wh_charge, energy_wh_discharge, soc_wh and
        the self_consumption and self_sufficiency ratios, [n_intervals, n] each."""
        return self._table_watts("storage")

    # ------------------------------------------------------------------ the battery kind
    def enable_battery(self, n_steps, interval_s=900, *, capacity_wh=None, charge_w=None, discharge_w=None, charge_eff=1.0,
                       discharge_eff=1.0, standby_w=0.0, soc0_wh=0.0, step0=None, buffer=None, soc=None, params=None):
        """enable_storage with losses and per-chain batteries (tmhpvsim_amd.battery): each chain's battery has
        its own capacity, charge and discharge limits (at the meter side), charge and discharge efficiency
        (floats in [0.5, 1]) and standby drain, each argument a scalar or [n]; a capacity of 0 is a household
        without a battery.  Returns the raw int64 tensor [n_intervals, 10, n]: storage's nine columns
        (charged and discharged at the meter side) and the loss.  `sim.soc` is the int64 state of charge [n],
        `sim.battery_params` the int64 parameters [6, n] on the device (battery.quantize_params).  params: a
        ready int64 device tensor [6, n] instead of the six quantities -- it may be a column slice of a
        larger [6, N] one whose row stride is the table's ld (buffer a slice of [n_intervals, 10, N]), and
        its values must lie in battery.RANGES (checked here; the kernels clamp).  soc0_wh must lie in
        [0, capacity]; a caller's soc tensor is clamped into it by the first window.  buffer, soc, step0,
        fp64 only, no traces, no fleet series, no other table, compaction: as enable_storage.  n_steps=None
        switches the output off."""
        if n_steps is None and self._battery_fleet is not None:   # (the kind's own output: off with it)
            self.enable_battery_fleet(None)

        def quantize():
            if capacity_wh is None or charge_w is None or discharge_w is None:
                raise ValueError("enable_battery: capacity_wh, charge_w and discharge_w (or params) are required")
            from . import battery
            return battery.quantize_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w, n=self.n)
        return self._enable_battery("battery", n_steps, interval_s, step0, buffer, soc, params, soc0_wh, quantize)

    def battery(self):
        """The battery table in watts and watt-hours (battery.to_watts of battery_raw): storage's keys plus
        energy_wh_loss and round_trip, [n_intervals, n] each."""
        return self._table_watts("battery")

    # ------------------------------------------------------------------ battery dispatch
    def enable_dispatch(self, n_steps, interval_s=900, *, capacity_wh=None, charge_w=None, discharge_w=None, charge_eff=1.0,
                        discharge_eff=1.0, standby_w=0.0, charge_above_w=0.0, discharge_above_w=0.0, feed_in_limit_w=None,
                        soc0_wh=0.0, params=None, soc=None, buffer=None, step0=None):
        """enable_battery under another control rule than greedy self-consumption (tmhpvsim_amd.dispatch): each
        chain's battery charges only from the surplus above charge_above_w, discharges only into the deficit
        above discharge_above_w, and what is left of the surplus is fed in up to feed_in_limit_w (None: no
        limit), the rest curtailed; each quantity a scalar or [n].  Returns the raw int64 tensor
        [n_intervals, 13, n]: the battery kind's ten columns (the export after the limit), the curtailed energy
        and the peak import and peak feed-in behind the battery as demand keys.  `sim.soc` is the int64 state
        of charge [n], `sim.dispatch_params` the int64 parameters [9, n] on the device
        (dispatch.quantize_params).  params: a ready int64 device tensor [9, n] instead of the quantities -- it
        may be a column slice of a larger [9, N] one whose row stride is the table's ld (buffer a slice of
        [n_intervals, 13, N]); its values must lie in dispatch.RANGES (checked here; the kernels clamp).
        soc0_wh, soc, buffer, step0, fp64 only, no traces, no fleet series, no battery fleet series, no other
        table, compaction: as enable_battery.  n_steps=None switches the output off."""
        def quantize():
            if capacity_wh is None or charge_w is None or discharge_w is None:
                raise ValueError("enable_dispatch: capacity_wh, charge_w and discharge_w (or params) are required")
            from . import dispatch
            return dispatch.quantize_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w,
                                            charge_above_w, discharge_above_w, feed_in_limit_w, n=self.n)
        return self._enable_battery("dispatch", n_steps, interval_s, step0, buffer, soc, params, soc0_wh, quantize)

    def dispatch(self):
        """The dispatch table in watts and watt-hours (dispatch.to_watts of dispatch_raw): the battery kind's keys
        plus energy_wh_curtailed, curtailed_share and the peaks behind the battery, [n_intervals, n] each."""
        return self._table_watts("dispatch")

    # ------------------------------------------------------------------ scheduled dispatch
    def enable_schedule(self, n_steps, interval_s=900, *, capacity_wh=None, charge_w=None, discharge_w=None, charge_eff=1.0,
                        discharge_eff=1.0, standby_w=0.0, rules=None, params=None, rule_of_interval=None, n_rules=None,
                        soc0_wh=0.0, soc=None, buffer=None, step0=None):
        """enable_dispatch with a rule that changes at known times (tmhpvsim_amd.schedule): each chain has one
        battery and R <= schedule.RULES_MAX rule sets -- `rules`, a list of dicts with charge_above_w,
        discharge_above_w, feed_in_limit_w (None: no limit) and grid_charge_w (the power the battery also takes from
        the grid; a grid-charging rule never discharges), each a scalar or [n] -- and rule_of_interval, a uint8
        sequence, array or device tensor [n_intervals] shared by all chains, names the rule in force in each
        metering interval of the table (schedule.daily builds one from a daily local-time tariff).  Returns the raw
        int64 tensor [n_intervals, 13, n], battery dispatch's columns.  `sim.soc` is the int64 state of charge [n],
        `sim.schedule_params` the int64 parameters [6 + 4 R, n] and `sim.schedule_rules` the uint8 array on the
        device.  params: a ready int64 device tensor [6 + 4 R, n] instead of the quantities and `rules` -- it may be a
        column slice of a wider one whose row stride is the table's ld; its values must lie in their ranges
        (schedule.check_params; the kernels clamp).  n_rules, when given, is checked against R; entries of
        rule_of_interval at or above R are refused (schedule.check_rules).  soc0_wh, soc, buffer, step0, fp64 only, no
        traces, no fleet series, no battery fleet series, no other table, compaction: as enable_dispatch; per-chain
        sites are refused.  A refused call leaves what was enabled before as it was.  n_steps=None switches the
        output off."""
        from . import schedule

        def quantize():
            if capacity_wh is None or charge_w is None or discharge_w is None or rules is None:
                raise ValueError("enable_schedule: capacity_wh, charge_w, discharge_w and rules (or params) are required")
            return schedule.quantize_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w,
                                            rules=rules, n=self.n)

        def last(host):   # the rule array of the table's intervals on the device, and the rule count
            torch = _torch()
            R = schedule.n_rules_of(host)
            if n_rules is not None and int(n_rules) != R:
                raise ValueError(f"enable_schedule: n_rules {int(n_rules)} but the schedule params hold {R} rules")
            if rule_of_interval is None:
                raise ValueError("enable_schedule: the schedule needs rule_of_interval (the rule of each metering interval)")
            nk = schedule.n_intervals(int(n_steps), int(interval_s))
            if torch.is_tensor(rule_of_interval):
                if rule_of_interval.dtype != torch.uint8 or rule_of_interval.dim() != 1:
                    raise ValueError("schedule rule_of_interval must be a uint8 [n_intervals] array")
                schedule.check_rules(rule_of_interval, R, nk)
                return rule_of_interval.to(self.device).contiguous(), R
            a = np.asarray(rule_of_interval)
            if a.dtype != np.uint8:
                if a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) > 255)):
                    raise ValueError("schedule rule_of_interval must hold integers in [0, 255]")
                a = a.astype(np.uint8)
            return torch.from_numpy(np.ascontiguousarray(schedule.check_rules(a, R, nk))).to(self.device), R
        raw = self._enable_battery("schedule", n_steps, interval_s, step0, buffer, soc, params, soc0_wh, quantize, last=last)
        if n_steps is not None:
            self.schedule_rules = self._battery_args[2][0]
        return raw

    def schedule(self):
        """The schedule table in watts and watt-hours (schedule.to_watts of schedule_raw): battery dispatch's keys,
        [n_intervals, n] each."""
        return self._table_watts("schedule")

    # ------------------------------------------------------------------ the battery sweep
    def enable_battery_sweep(self, n_steps, interval_s=900, *, n_variants=None, capacity_wh=None, charge_w=None,
                             discharge_w=None, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, soc0_wh=0.0, step0=None,
                             buffer=None, soc=None, params=None):
        """enable_battery for K candidate batteries per chain in one run (tmhpvsim_amd.battery, tmh_battery_sweep):
        every chain -- the same pv and meter second for second -- behind each of K batteries, variant v's table
        and state of charge bit for bit what enable_battery gives for its parameters.  Each quantity is a scalar,
        a sequence of K values (one per variant, uniform over the chains) or a [K, n] array
        (battery.quantize_sweep_params); or pass params, a ready int64 device tensor [K, 6, n] (checked with
        battery.check_params per variant).  Returns the raw int64 tensor [K, n_intervals, 10, n];
        `sim.soc` is the int64 [K, n] state of charge, `sim.battery_params` the parameters [K, 6, n].  buffer,
        soc, params: tensors of those shapes to use, possibly column slices of wider [.., N] tensors of one width.
        fp64 only, no traces, no fleet series, no battery fleet series, no other table, no per-chain sites;
        compaction is allowed.  n_steps=None switches the output off."""
        def quantize():
            if capacity_wh is None or charge_w is None or discharge_w is None:
                raise ValueError("enable_battery_sweep: capacity_wh, charge_w and discharge_w (or params) are required")
            from . import battery
            return battery.quantize_sweep_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w,
                                                 n=self.n, n_variants=n_variants)
        return self._enable_battery("battery_sweep", n_steps, interval_s, step0, buffer, soc, params, soc0_wh, quantize,
                                    n_variants=n_variants)

    def battery_sweep(self):
        """The sweep's tables in watts and watt-hours: a list of battery.to_watts dicts, one per variant."""
        from .battery import to_watts
        if self.battery_sweep_raw is None:
            raise ValueError("no battery sweep tables: call enable_battery_sweep first")
        _torch().cuda.synchronize(self.device)
        t = self._battery_sweep
        return [to_watts(raw, t.interval_s, n_steps=t.n_steps) for raw in self.battery_sweep_raw]

    # ------------------------------------------------------------------ the dispatch sweep
    def enable_dispatch_sweep(self, n_steps, interval_s=900, *, n_variants=None, capacity_wh=None, charge_w=None,
                              discharge_w=None, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, charge_above_w=0.0,
                              discharge_above_w=0.0, feed_in_limit_w=None, soc0_wh=0.0, step0=None, buffer=None, soc=None,
                              params=None):
        """enable_dispatch for K rule sets per chain in one run (tmhpvsim_amd.dispatch, tmh_dispatch_sweep): every
        chain -- the same pv and meter second for second -- under each of K sets of battery, thresholds and
        feed-in limit, variant v's table and state of charge bit for bit what enable_dispatch gives for its
        parameters.  Each quantity is a scalar, a sequence of K values (one per variant, uniform over the chains)
        or a [K, n] array; feed_in_limit_w entries may be None (dispatch.quantize_sweep_params); or pass params, a
        ready int64 device tensor [K, 9, n] (checked with dispatch.check_params per variant).  Returns the raw
        int64 tensor [K, n_intervals, 13, n]; `sim.soc` is the int64 [K, n] state of charge, `sim.dispatch_params`
        the parameters [K, 9, n].  buffer, soc, params: tensors of those shapes to use, possibly column slices of
        wider [.., N] tensors of one width.  fp64 only, no traces, no fleet series, no battery fleet series, no
        other table, no per-chain sites; compaction is allowed.  n_steps=None switches the output off."""
        def quantize():
            if capacity_wh is None or charge_w is None or discharge_w is None:
                raise ValueError("enable_dispatch_sweep: capacity_wh, charge_w and discharge_w (or params) are required")
            from . import dispatch
            return dispatch.quantize_sweep_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w,
                                                  charge_above_w, discharge_above_w, feed_in_limit_w, n=self.n,
                                                  n_variants=n_variants)
        return self._enable_battery("dispatch_sweep", n_steps, interval_s, step0, buffer, soc, params, soc0_wh, quantize,
                                    n_variants=n_variants)

    def dispatch_sweep(self):
        """The sweep's tables in watts and watt-hours: a list of dispatch.to_watts dicts, one per variant."""
        from .dispatch import to_watts
        if self.dispatch_sweep_raw is None:
            raise ValueError("no dispatch sweep tables: call enable_dispatch_sweep first")
        _torch().cuda.synchronize(self.device)
        t = self._dispatch_sweep
        return [to_watts(raw, t.interval_s, n_steps=t.n_steps) for raw in self.dispatch_sweep_raw]

    # ------------------------------------------------------------------ the schedule sweep
    def enable_schedule_sweep(self, n_steps, interval_s=900, *, n_variants=None, capacity_wh=None, charge_w=None,
                              discharge_w=None, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, rules=None, params=None,
                              rule_of_interval=None, n_rules=None, soc0_wh=0.0, soc=None, buffer=None, step0=None):
        """enable_schedule for K variants per chain in one run (tmhpvsim_amd.schedule, tmh_schedule_sweep): every
        chain -- the same pv and meter second for second -- under each of K sets of battery, R rule sets and rule
        array, variant v's table and state of charge bit for bit what enable_schedule gives for its parameters and
        its array: which tariff a household should take, whether grid charging at night pays under it, which battery
        to buy.  Each battery quantity and each value in `rules` (enable_schedule's list of R dicts) is a scalar, a
        sequence of K values (one per variant, uniform over the chains) or a [K, n] array; feed-in limits may be None
        (schedule.quantize_sweep_params); or pass params, a ready int64 device tensor [K, 6 + 4 R, n]
        (schedule.check_sweep_params).  rule_of_interval is a uint8 sequence, array or device tensor [n_intervals]
        (every variant's) or [K, n_intervals] (a tariff per variant: schedule.check_sweep_rules); n_rules, when
        given, is checked against R.  Returns the raw int64 tensor [K, n_intervals, 13, n]; `sim.soc` is the int64
        [K, n] state of charge, `sim.schedule_sweep_params` the parameters [K, 6 + 4 R, n] and
        `sim.schedule_sweep_rules` the uint8 arrays [K, n_intervals] on the device.  buffer, soc, params: tensors of
        those shapes to use, possibly column slices of wider [.., N] tensors of one width.  fp64 only, no traces, no
        fleet series of any kind, no other table, no per-chain sites; compaction is allowed.  A refused call leaves
        what was enabled before as it was.  n_steps=None switches the output off."""
        from . import schedule

        def quantize():
            if capacity_wh is None or charge_w is None or discharge_w is None or rules is None:
                raise ValueError("enable_schedule_sweep: capacity_wh, charge_w, discharge_w and rules (or params) are required")
            return schedule.quantize_sweep_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w,
                                                  rules=rules, n=self.n, n_variants=n_variants)

        def last(host):   # the variants' rule arrays of the table's intervals on the device, and the rule count
            torch = _torch()
            K, R = int(host.shape[0]), schedule.n_rules_of(host[0])
            if n_rules is not None and int(n_rules) != R:
                raise ValueError(f"enable_schedule_sweep: n_rules {int(n_rules)} but the schedule sweep params hold {R} rules")
            if rule_of_interval is None:
                raise ValueError("enable_schedule_sweep: the schedule sweep needs rule_of_interval (the rule of each metering "
                                 "interval, [n_intervals] or [K, n_intervals])")
            a = rule_of_interval.cpu().numpy() if torch.is_tensor(rule_of_interval) else np.asarray(rule_of_interval)
            if a.dtype != np.uint8:
                if torch.is_tensor(rule_of_interval):
                    raise ValueError("schedule sweep rule_of_interval must be a uint8 [n_intervals] or [K, n_intervals] array")
                if a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) > 255)):
                    raise ValueError("schedule sweep rule_of_interval must hold integers in [0, 255]")
                a = a.astype(np.uint8)
            a = schedule.check_sweep_rules(a, R, schedule.n_intervals(int(n_steps), int(interval_s)), K)
            return torch.from_numpy(a).to(self.device), R
        if n_steps is not None and self._dispatch_fleet is not None:
            raise ValueError("a dispatch fleet series is enabled: it is battery dispatch's or the schedule's "
                             "(the schedule sweep runs alone)")
        raw = self._enable_battery("schedule_sweep", n_steps, interval_s, step0, buffer, soc, params, soc0_wh, quantize,
                                   n_variants=n_variants, last=last)
        if n_steps is not None:
            self.schedule_sweep_rules = self._battery_args[2][0]
        return raw

    def schedule_sweep(self):
        """Per variant and chain over the run (schedule.sweep_summary of schedule_sweep_raw and the parameters):
        dispatch.sweep_summary's keys, float64 [K, n] each."""
        from .schedule import sweep_summary
        if self.schedule_sweep_raw is None:
            raise ValueError("no schedule sweep tables: call enable_schedule_sweep first")
        _torch().cuda.synchronize(self.device)
        return sweep_summary(self.schedule_sweep_raw, self._schedule_sweep.interval_s, self.schedule_sweep_params)

    # ------------------------------------------------------------------ the battery fleet series
    def enable_battery_fleet(self, n_steps, step0=None, group_chains=0, buffer=None):
        """Beside the battery kind's table (enable_battery first), accumulate the battery fleet series
        (tmhpvsim_amd.battery.FLEET_COLUMNS: per second and group of chains, the fleet series' four columns and
        the exact integer sums of the import and the export behind the batteries, of the state of charge after
        the second and of what the batteries take) of steps [step0, step0 + n_steps) in every later run.
        step0, group_chains and buffer as enable_series, with rows of eight: `sim.battery_fleet_raw` is the
        int64 tensor [n_groups, n_steps, 8] (several sims may add into one buffer).  run() and its window
        pipeline carry it; compact=True is refused.  n_steps=None switches it off; so does
        enable_battery(None)."""
        torch = _torch()
        if n_steps is None:
            _lib.check(self.L.tmh_set_battery_fleet(self._eng, None))
            self.battery_fleet_raw, self._battery_fleet = None, None
            return None
        if self._battery is None:
            raise ValueError("enable_battery_fleet: call enable_battery first (the battery kind's replay pass fills "
                             "the battery fleet series)")
        from .battery import FLEET_COLUMNS
        n_steps, gc, nc = int(n_steps), int(group_chains), len(FLEET_COLUMNS)
        if n_steps < 1 or gc < 0 or gc % 512:
            raise ValueError("enable_battery_fleet: n_steps >= 1, group_chains 0 or a multiple of 512")
        n_groups = 1 if gc == 0 else -(-self.n // gc)
        if buffer is None:
            buffer = torch.zeros(n_groups, n_steps, nc, dtype=torch.int64, device=self.device)
        elif (buffer.dtype != torch.int64 or buffer.device != self.device or not buffer.is_contiguous()
              or buffer.dim() != 3 or buffer.shape[0] < n_groups or tuple(buffer.shape[1:]) != (n_steps, nc)):
            raise ValueError(f"battery fleet buffer must be a contiguous int64 [>= {n_groups}, {n_steps}, {nc}] tensor "
                             f"on {self.device}")
        st = _lib.Series(buffer.data_ptr(), self.step if step0 is None else int(step0), n_steps, gc,
                         int(buffer.shape[0]), 0)
        _lib.check(self.L.tmh_set_battery_fleet(self._eng, C.byref(st)))
        self.battery_fleet_raw, self._battery_fleet = buffer, st
        return buffer

    def battery_fleet(self, bin_s=1, mean=False):
        """The battery fleet series in watts and watt-hours (battery.fleet_to_watts of battery_fleet_raw),
        [n_groups, n_bins] each."""
        from .battery import fleet_to_watts
        if self.battery_fleet_raw is None:
            raise ValueError("no battery fleet series: call enable_battery_fleet first")
        _torch().cuda.synchronize(self.device)
        return fleet_to_watts(self.battery_fleet_raw, bin_s=bin_s, mean=mean)

    # ------------------------------------------------------------------ the dispatch fleet series
    def enable_dispatch_fleet(self, n_steps, step0=None, group_chains=0, buffer=None):
        """Beside battery dispatch's or the schedule's table (enable_dispatch or enable_schedule first), accumulate
        the dispatch fleet series (tmhpvsim_amd.dispatch.FLEET_COLUMNS: per second and group of chains, the battery
        fleet series' eight columns under the kind's rule -- the export after the feed-in limit, the import with
        what a grid-charging rule buys -- and the curtailed power) of steps [step0, step0 + n_steps) in every later
        run: the feeder's coincident peaks, which no table holds.  step0, group_chains and buffer as
        enable_battery_fleet, with rows of nine: `sim.dispatch_fleet_raw` is the int64 tensor [n_groups, n_steps, 9]
        (several sims may add into one buffer).  The kind's table and `sim.soc` are what they are without the
        series.  run() and its window pipeline carry it; compact=True and per-chain sites are refused.
        n_steps=None switches it off; so does switching the kind off."""
        torch = _torch()
        if n_steps is None:
            _lib.check(self.L.tmh_set_dispatch_fleet(self._eng, None))
            self.dispatch_fleet_raw, self._dispatch_fleet = None, None
            return None
        if self._dispatch is None and self._schedule is None:
            raise ValueError("enable_dispatch_fleet: call enable_dispatch or enable_schedule first (the kind's replay pass "
                             "fills the dispatch fleet series)")
        if self.sites is not None:
            raise ValueError("a dispatch fleet series cannot run with per-chain sites (one feeder is one site)")
        from .dispatch import FLEET_COLUMNS
        n_steps, gc, nc = int(n_steps), int(group_chains), len(FLEET_COLUMNS)
        if n_steps < 1 or gc < 0 or gc % 512:
            raise ValueError("enable_dispatch_fleet: n_steps >= 1, group_chains 0 or a multiple of 512")
        n_groups = 1 if gc == 0 else -(-self.n // gc)
        if buffer is None:
            buffer = torch.zeros(n_groups, n_steps, nc, dtype=torch.int64, device=self.device)
        elif (buffer.dtype != torch.int64 or buffer.device != self.device or not buffer.is_contiguous()
              or buffer.dim() != 3 or buffer.shape[0] < n_groups or tuple(buffer.shape[1:]) != (n_steps, nc)):
            raise ValueError(f"dispatch fleet buffer must be a contiguous int64 [>= {n_groups}, {n_steps}, {nc}] tensor "
                             f"on {self.device}")
        st = _lib.Series(buffer.data_ptr(), self.step if step0 is None else int(step0), n_steps, gc,
                         int(buffer.shape[0]), 0)
        _lib.check(self.L.tmh_set_dispatch_fleet(self._eng, C.byref(st)))
        self.dispatch_fleet_raw, self._dispatch_fleet = buffer, st
        return buffer

    def dispatch_fleet(self, bin_s=1, mean=False):
        """The dispatch fleet series in watts and watt-hours (dispatch.fleet_to_watts of dispatch_fleet_raw),
        [n_groups, n_bins] each; dispatch.fleet_peaks gives the bins' coincident peaks."""
        from .dispatch import fleet_to_watts
        if self.dispatch_fleet_raw is None:
            raise ValueError("no dispatch fleet series: call enable_dispatch_fleet first")
        _torch().cuda.synchronize(self.device)
        return fleet_to_watts(self.dispatch_fleet_raw, bin_s=bin_s, mean=mean)

    def guard_records(self):
        """Tests: the fp32 guard-band records (chain, 128-s block) of the last window that run()
        issued as a single tmh_run (tmh_test_guard_records; synchronises the device)."""
        if self._last_scratch is None:
            raise ValueError("no single-window run yet")
        ws, off, k = self._last_scratch
        _torch().cuda.synchronize(self.device)
        r = self.L.tmh_test_guard_records(self._eng, C.c_void_p(ws.data_ptr() + off), self.n, k)
        if r < 0:
            _lib.check(int(r))
        return int(r)

    # ------------------------------------------------------------------ run
    def workspace(self, n_steps):
        """plan + scratch of one window (tmh_engine_scratch_bytes: this engine's precision).  The
        plan part is written by tmh_plan only and must stay unchanged until the window's expansion
        has finished (the expansion reads it as constant memory)."""
        nb = self.L.tmh_plan_bytes(n_steps) + self.L.tmh_engine_scratch_bytes(self._eng, self.n, n_steps)
        return _torch().empty(nb, dtype=torch_uint8(), device=self.device)

    def run(self, n_steps, trace=TRACE_FIELDS, window=86400, out=None, compact=False):
        """Advance n_steps seconds.  Returns {field: tensor[n_steps, n_chains]} for `trace`.

        compact=True (statistics runs, trace=()): each window after the first runs
        on the chains still live at its start only (tmh_live_chains, tmh_state_move,
        tmh_set_chain_ids), so chains the reference's AssertionError ended
        (cloud_cover_binary.py:91; most C5 chains within the week) cost nothing
        more.  Every chain's state and statistics come out as without compaction.
        `compact_slots` then lists the slots (chains still live) each window of the
        run ran on, the first always n."""
        torch = _torch()
        n_steps = int(n_steps)
        trace = tuple(trace or ())
        if compact and (trace or self._us is not None):
            raise ValueError("compact=True needs a keyed statistics run (trace=(), no injected uniforms)")
        if self._series is not None:   # (the library refuses each too, window by window)
            if compact:
                raise ValueError("a fleet series cannot run compacted (a compacted tile would mix groups)")
            if trace:
                raise ValueError("a fleet series run takes no traces (trace=()): sum the traces instead "
                                 "(series.from_traces)")
            s0, sn = self._series.step0, self._series.n_steps
            if self.step < s0 or self.step + n_steps > s0 + sn:
                raise ValueError(f"steps [{self.step}, +{n_steps}) outside the series [{s0}, +{sn})")
        for kind, t in _TABLES.items():   # (likewise; compact=True is allowed)
            tb = getattr(self, "_" + kind)
            if tb is None:
                continue
            if self._series is not None:
                raise ValueError(f"{t['name']} and a fleet series are both enabled: one of the two per sim")
            if t["run_excludes"] and any(getattr(self, attr) is not None for attr in t["run_excludes"][0]):
                raise ValueError(t["run_excludes"][1])
            if trace:
                raise ValueError(t["no_trace"])
            if self.step < tb.step0 or self.step + n_steps > tb.step0 + tb.n_steps:
                raise ValueError(f"steps [{self.step}, +{n_steps}) outside the {t['noun']} [{tb.step0}, +{tb.n_steps})")
        if self._battery_fleet is not None:   # (the library refuses each too, window by window)
            if compact:
                raise ValueError("a battery fleet series cannot run compacted (a compacted tile would mix groups)")
            s0, sn = self._battery_fleet.step0, self._battery_fleet.n_steps
            if self.step < s0 or self.step + n_steps > s0 + sn:
                raise ValueError(f"steps [{self.step}, +{n_steps}) outside the battery fleet series [{s0}, +{sn})")
        if self._dispatch_fleet is not None:   # (likewise)
            if compact:
                raise ValueError("a dispatch fleet series cannot run compacted (a compacted tile would mix groups)")
            if trace:
                raise ValueError("a dispatch fleet series run takes no traces (trace=()): run the rule over the traces "
                                 "instead (dispatch.fleet_from_traces)")
            s0, sn = self._dispatch_fleet.step0, self._dispatch_fleet.n_steps
            if self.step < s0 or self.step + n_steps > s0 + sn:
                raise ValueError(f"steps [{self.step}, +{n_steps}) outside the dispatch fleet series [{s0}, +{sn})")
        if n_steps > ROLL_MAX:   # one rolling clock covers at most ROLL_MAX steps: run in pieces (same bits)
            res = out if out is not None else self._alloc(n_steps, trace)
            done = 0
            while done < n_steps:
                k = min(ROLL_MAX, n_steps - done)
                self.run(k, trace, window, {f: res[f][done:done + k] for f in trace}, compact=compact)
                done += k
            return res
        if self.step + n_steps > self.clock.end:
            self._roll(n_steps)
        for f in trace:
            if f not in TRACE_FIELDS:
                raise ValueError(f"unknown trace field {f!r}")
        res = out if out is not None else self._alloc(n_steps, trace)
        st = self._stats_struct()
        win = max(1, min(int(window), n_steps))
        self._work_window(win)
        if compact and n_steps > win:
            with torch.cuda.device(self.device):
                self._run_compacted(n_steps, win, st)
            self.step += n_steps
            return res
        if self.path == "time_parallel" and n_steps > win:
            with torch.cuda.device(self.device):
                self._run_pipelined(n_steps, win, trace, res, st)
            self.step += n_steps
            return res
        ws = self.workspace(win)
        with torch.cuda.device(self.device):
            done = 0
            while done < n_steps:
                k = min(win, n_steps - done)
                tr = _lib.Trace(*(res[f][done:done + k].data_ptr() if f in trace else None
                                  for f in ("csi", "covered", "pv", "meter", "residual")), self.n)
                _lib.check(self.L.tmh_run(self._eng, _ptr(self.state), self.chain0, self.n, self.step + done, k,
                                          C.byref(self._us) if self._us is not None else None,
                                          C.byref(tr), C.byref(st) if st is not None else None,
                                          _ptr(ws), ws.numel(), self._stream()))
                self._last_scratch = (ws, int(self.L.tmh_plan_bytes(k)), k)
                done += k
        self.step += n_steps
        return res

    def _run_compacted(self, n_steps, win, st):
        """Windows in order; from the second on, only the chains live at the window
        start run, gathered into a dense working state and scattered back after it."""
        torch = _torch()
        L, s = self.L, self._stream()
        ws = self.workspace(win)
        work = torch.empty_like(self.state)
        ids = torch.empty(self.n, dtype=torch.int32, device=self.device)
        nlive = torch.zeros(1, dtype=torch.int32, device=self.device)
        tr = _lib.Trace(None, None, None, None, None, self.n)
        self.compact_slots = []
        done = 0
        while done < n_steps:
            k = min(win, n_steps - done)
            nl, cur = self.n, self.state
            if done > 0:
                _lib.check(L.tmh_live_chains(self._eng, _ptr(self.state), self.n, None, _ptr(ids), _ptr(nlive), s))
                nl = int(nlive.item())
                if nl < self.n:
                    cur = work
                    if nl:
                        _lib.check(L.tmh_state_move(self._eng, _ptr(self.state), self.n, _ptr(work), nl, _ptr(ids),
                                                    _ptr(nlive), nl, 0, s))
                        _lib.check(L.tmh_set_chain_ids(self._eng, _ptr(ids), self.n))
            self.compact_slots.append(nl)
            try:
                if nl:
                    _lib.check(L.tmh_run(self._eng, _ptr(cur), self.chain0, nl, self.step + done, k, None, C.byref(tr),
                                         C.byref(st) if st is not None else None, _ptr(ws), ws.numel(), s))
                if nl and cur is work:
                    _lib.check(L.tmh_state_move(self._eng, _ptr(work), nl, _ptr(self.state), self.n, _ptr(ids),
                                                _ptr(nlive), nl, 1, s))
            finally:
                _lib.check(L.tmh_set_chain_ids(self._eng, None, 0))
            done += k

    def _alloc(self, n_steps, trace):
        torch = _torch()
        return {f: torch.empty(n_steps, self.n, dtype=torch.uint8 if f == "covered" else self.real, device=self.device)
                for f in trace}

    def _roll(self, n_steps):
        """The next rolling wall clock, from the current step (tmh_set_clock)."""
        self.clock = make_clock(self._start, max(int(n_steps), min(self.horizon, ROLL_MAX)), self._tz, step0=self.step)
        _lib.check(self.L.tmh_set_clock(self._eng, C.byref(self.clock.as_struct())))

    def _run_pipelined(self, n_steps, win, trace, res, st):
        """Windows of the time-parallel path, pipelined (run_windows): each window's plan,
        draws and segment walk on a walk stream that runs up to two windows ahead of the
        expansions on the current stream.  Same bits as one tmh_run per window
        (tests/test_gpu_parity.py)."""
        torch = _torch()
        main = torch.cuda.current_stream(self.device)
        if getattr(self, "_wstream", None) is None:
            self._wstream = torch.cuda.Stream(self.device, priority=torch.cuda.Stream.priority_range()[1])
            self._pstream = torch.cuda.Stream(self.device)
        wins = []
        done = 0
        while done < n_steps:
            k = min(win, n_steps - done)
            wins.append((self.step + done, k, done))
            done += k
        bufs = [self.workspace(win) for _ in range(min(WINDOW_BUFFERS, len(wins)))]

        def trace_of(w):
            off, k = wins[w][2], wins[w][1]
            return _lib.Trace(*(res[f][off:off + k].data_ptr() if f in trace else None
                                for f in ("csi", "covered", "pv", "meter", "residual")), self.n)

        run_windows(self.L, self._eng, self.state, self.chain0, self.n, [(a, k) for a, k, _ in wins], bufs, main,
                    self._wstream, trace_of, st, plan_stream=self._pstream)
        self._keep = bufs   # allocated on the main stream, whose last work is the last expansion

    def plan(self, step0, n_steps):
        """Build the chain-independent plan of a window (tmh_plan); returns the uint8 buffer."""
        torch = _torch()
        plan = torch.empty(self.L.tmh_plan_bytes(int(n_steps)), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.tmh_plan(self._eng, int(step0), int(n_steps), _ptr(plan), self._stream()))
        return plan

    def geometry(self, step0, n_steps):
        """The clock/geometry table rows [n_steps, TMH_GEOM_FIELDS] (fp64) of a window."""
        torch = _torch()
        plan = self.plan(step0, n_steps)
        return plan[: n_steps * _lib.TMH_GEOM_FIELDS * 8].view(torch.float64).view(n_steps, _lib.TMH_GEOM_FIELDS)

    def probe_pv(self, rows, csi):
        """The per-second PV chain on given geometry rows (tmh_probe_pv; parity tests): rows
        [n, TMH_GEOM_FIELDS] fp64 in geometry()'s layout, csi [n] -> numpy [n, 3]: the fp64 chain's
        power, the fp32 chain's on the row's fp32 form, and that second's guard-band flag (0 / 1)."""
        torch = _torch()
        rt = torch.as_tensor(np.asarray(rows, dtype=np.float64) if not torch.is_tensor(rows) else rows,
                             dtype=torch.float64, device=self.device).contiguous()
        ct = torch.as_tensor(np.asarray(csi, dtype=np.float64) if not torch.is_tensor(csi) else csi,
                             dtype=torch.float64, device=self.device).contiguous()
        if rt.dim() != 2 or rt.shape[1] != _lib.TMH_GEOM_FIELDS or tuple(ct.shape) != (rt.shape[0],):
            raise ValueError(f"probe_pv wants rows [n, {_lib.TMH_GEOM_FIELDS}] and csi [n], got "
                             f"{tuple(rt.shape)} and {tuple(ct.shape)}")
        out = torch.empty(rt.shape[0], 3, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.tmh_probe_pv(self._eng, _ptr(rt), _ptr(ct), _ptr(out), rt.shape[0], self._stream()))
            torch.cuda.synchronize()
        return out.cpu().numpy()

    def stats_totals(self):
        """Node-local totals: histogram, energy sums (W*s, exact fixed-point limbs and the
        fp64 values of them) and peak residual (W) over every chain's accumulated
        seconds -- a faulted chain's seconds before its fault included, in energies
        and histogram alike (dist.chain_totals)."""
        from .dist import chain_totals
        return chain_totals(self.chain_acc, self.hist.clone() if self.hist is not None else None)


WINDOW_BUFFERS = 3   # plan + scratch sets of the multi-window pipeline (run_windows)


def run_windows(L, eng, state, chain0, n, wins, bufs, main, walk, trace_of, st, plan_stream=None):
    """Consecutive windows [(step0, n_steps)] of the same chains, software-pipelined over
    len(bufs) workspace buffers (plan + scratch each, window w in buffer w % K):

      plan stream: plan(w) (chain-independent: clock and geometry rows) as soon as buffer
                   w % K is free;
      walk stream: draws(w) chained to window w-1's walk (tmh_walk_part with
                   prev_scratch), segment walk(w) -- up to K-1 windows ahead;
      main stream: expansion + commit of window w once its walk is done.

    The walk of a window needs only the previous window's walk (its end status,
    cloud-cover and wind pairs, call counts, sigma arrays), never its expansion, so the
    walks run back to back while the expansions follow; buffer w % K is reused once the
    expansion of window w - K is done -- and not before: a window's plan is read-only from
    its tmh_plan until its expansion has finished (the interval-metering expansion reads the
    plan's geometry rows as constant memory), so nothing may rewrite a plan buffer under a
    running expansion.  With small batches (the walk latency-bound) the
    per-window tail (fixup, commit, plan, draws) is off the walk's path.  trace_of(w):
    the window's tmh_trace; st: tmh_stats or None.  Same bits as one tmh_run per window."""
    import ctypes as C
    torch = _torch()
    K = len(bufs)
    pst = plan_stream or walk
    mptr, wptr, pptr = C.c_void_p(main.cuda_stream), C.c_void_p(walk.cuda_stream), C.c_void_p(pst.cuda_stream)
    nb = bufs[0].numel()
    pbytes = [L.tmh_plan_bytes(int(max(k for _, k in wins)))] * K
    walked = [torch.cuda.Event() for _ in range(K)]
    expanded = [torch.cuda.Event() for _ in range(K)]
    planned = [torch.cuda.Event() for _ in range(K)]

    def views(w):
        b = bufs[w % K]
        return C.c_void_p(b.data_ptr()), C.c_void_p(b.data_ptr() + pbytes[w % K]), nb - pbytes[w % K]

    def prev_of(w):
        return (views(w - 1)[1], wins[w - 1][1]) if w > 0 else (None, 0)

    def issue_walk(w):   # plan, draws and segment walk of window w, on the walk stream
        s0, k = wins[w]
        plan, scr, sb = views(w)
        if w >= K:
            pst.wait_event(expanded[w % K])    # the expansion of window w - K has read this buffer
            if pst is not walk:
                walk.wait_event(expanded[w % K])
        _lib.check(L.tmh_plan(eng, s0, k, plan, pptr))
        if pst is not walk:
            planned[w % K].record(pst)
            walk.wait_event(planned[w % K])
        ps, pk = prev_of(w)
        _lib.check(L.tmh_walk_part(eng, _ptr(state), chain0, n, s0, k, plan, scr, sb, ps, pk,
                                   _lib.WALK_DRAWS | _lib.WALK_SEGMENTS, wptr))
        walked[w % K].record(walk)

    # everything already issued on the main stream (the chains' construction, a previous
    # run's last commit) precedes this run's plans, draws and walks
    begun = torch.cuda.Event()
    begun.record(main)
    walk.wait_event(begun)
    if pst is not walk:
        pst.wait_event(begun)
    for w in range(min(K - 1, len(wins))):
        issue_walk(w)
    for w in range(len(wins)):
        if w + K - 1 < len(wins):
            issue_walk(w + K - 1)
        s0, k = wins[w]
        plan, scr, sb = views(w)
        main.wait_event(walked[w % K])
        tr = trace_of(w)
        _lib.check(L.tmh_expand(eng, _ptr(state), chain0, n, s0, k, None, C.byref(tr) if tr is not None else None,
                                C.byref(st) if st is not None else None, plan, scr, sb, mptr))
        expanded[w % K].record(main)


def torch_uint8():
    return _torch().uint8


def probe(fn, a, x, device="cuda"):
    """Device math probe (parity tests): fn 0 ndtri, 1 gammaincinv, 2 stdtrit, 3 al_ppf, 4 ndtri fp32,
    17 the segment walk's cloud-length power pow_d(x, a) (x = alpha + delta u, a = the exponent)."""
    torch = _torch()
    L = _lib.load()
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64), device=device)
    out = torch.empty_like(xt)
    _lib.check(L.tmh_probe(int(fn), float(a), _ptr(xt), _ptr(out), xt.numel(),
                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()
