"""The battery family's one host path (storage, the battery kind, battery dispatch, the schedule and the two sweeps):
which refusal a step gives when several apply, word for word, and the one work buffer that grows with the window."""
import ctypes as C

import numpy as np
import pytest

from storage_util import modules_params
from test_gpu_series import _np, _sim

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, WIN, IV = 64, 256, 60
START = "2019-09-05 10:00:00"   # daylight: the batteries charge
FAMILY = ("storage", "battery", "battery_sweep", "dispatch", "dispatch_sweep", "schedule")
COLS = dict(intervals=4, registers=6, demand=8, storage=9, battery=10, battery_sweep=10, dispatch=13, dispatch_sweep=13,
            schedule=13)


class _Rig:
    """A 64-chain fp64 engine with every kind's buffers valid for a 256-step window (so a step that is not refused
    runs a correct expansion), the kinds set and cleared through the C-ABI."""

    def __init__(self):
        from tmhpvsim_amd import _lib
        from tmhpvsim_amd.params import site_grid
        self.lib, self.sim = _lib, _sim(N, START, prec="fp64", horizon=1000)
        self.L = L = self.sim.L
        dev, K, nk = "cuda:0", 2, -(-WIN // IV)
        self.table = torch.zeros(K, nk, 13, N, dtype=torch.int64, device=dev)
        self.soc = torch.zeros(K, N, dtype=torch.int64, device=dev)
        self.params = torch.zeros(K, 6 + 4 * 2, N, dtype=torch.int64, device=dev)   # (capacity 0: no battery)
        self.rules = torch.zeros(nk, dtype=torch.uint8, device=dev)
        self.work = torch.zeros(L.tmh_battery_sweep_work_bytes(N, WIN, K), dtype=torch.uint8, device=dev)
        self.series = torch.zeros(1, WIN, 4, dtype=torch.int64, device=dev)
        self.fleet = torch.zeros(1, WIN, 8, dtype=torch.int64, device=dev)
        grid = site_grid(8, 8)
        self.sites = torch.from_numpy(np.ascontiguousarray(grid[0] if isinstance(grid, tuple) else grid, dtype=np.float64)).to(dev)
        self.ws = self.sim.workspace(WIN)
        self.pb = L.tmh_plan_bytes(WIN)
        self.plan()
        self.state0 = self.sim.state.clone()

    def plan(self):
        self.lib.check(self.L.tmh_plan(self.sim._eng, 0, WIN, C.c_void_p(self.ws.data_ptr()), None))
        torch.cuda.synchronize()

    def need(self, kind):
        return self.L.tmh_battery_sweep_work_bytes(N, WIN, 2 if kind.endswith("_sweep") else 1)

    def desc(self, kind, short=0):
        """kind's descriptor; short: bytes its work_bytes falls short of the window's."""
        _lib = self.lib
        tbl = _lib.Intervals(self.table.data_ptr(), 0, WIN, IV, N)
        if kind not in FAMILY:
            return tbl
        head = (tbl, self.soc.data_ptr(), self.work.data_ptr(), self.need(kind) - short)
        p = self.params.data_ptr()
        return {"storage": lambda: _lib.Storage(*head, 1000, 10, 10), "battery": lambda: _lib.Battery(*head, p),
                "battery_sweep": lambda: _lib.BatterySweep(*head, p, 2), "dispatch": lambda: _lib.Dispatch(*head, p),
                "dispatch_sweep": lambda: _lib.DispatchSweep(*head, p, 2),
                "schedule": lambda: _lib.Schedule(*head, p, self.rules.data_ptr(), 2)}[kind]()

    def set(self, kind, on=True, short=0):
        arg = C.byref(self.desc(kind, short)) if on else None
        self.lib.check(getattr(self.L, "tmh_set_" + kind)(self.sim._eng, arg))

    def set_series(self, which, on=True):
        buf = self.series if which == "series" else self.fleet
        arg = C.byref(self.lib.Series(buf.data_ptr(), 0, WIN, 0, 1, 0)) if on else None
        self.lib.check(getattr(self.L, "tmh_set_" + which)(self.sim._eng, arg))

    def set_sites(self, on=True):
        self.lib.check(self.L.tmh_set_sites(self.sim._eng, C.c_void_p(self.sites.data_ptr()) if on else None, None,
                                            N if on else 0))
        self.plan()   # (a plan is its engine's, sites included)

    def step(self):
        """tmh_step of the window: the refusal's text, or None when the step ran (the state is put back)."""
        sim, L = self.sim, self.L
        tr = self.lib.Trace(None, None, None, None, None, N)
        rc = L.tmh_step(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, N, 0, WIN, None, C.byref(tr), None,
                        C.c_void_p(self.ws.data_ptr()), C.c_void_p(self.ws.data_ptr() + self.pb),
                        self.ws.numel() - self.pb, None)
        if rc == 0:
            torch.cuda.synchronize()
            sim.state.copy_(self.state0)
            return None
        assert rc == -1
        return L.tmh_last_error().decode()


def _refusals():
    rig = _Rig()
    got = {}
    for a in FAMILY:
        for b in COLS:
            if b == a:
                continue
            for first, second in ((a, b), (b, a)):   # two kinds on one engine, in either order
                rig.set(first)
                rig.set(second)
                got[f"{first}, then {second}"] = rig.step()
                rig.set(a, False)
                rig.set(b, False)
        rig.set(a)
        for which in ("series", "battery_fleet"):
            rig.set_series(which)
            got[f"{a} beside a {which}"] = rig.step()
            rig.set_series(which, False)
        rig.set_sites()
        got[f"{a} with per-chain sites"] = rig.step()
        rig.set_sites(False)
        rig.set(a, short=1)
        got[f"{a}, work buffer one byte short"] = rig.step()
        rig.set(a, False)
    return got


# tmh_last_error() of the library built from commit d967865 (before the kinds' refusals became one check), case by
# case; None: the step is not refused (the battery kind fills the battery fleet series; storage, the battery kind and
# battery dispatch run with per-chain sites)
EXPECTED = {'storage, then intervals': 'battery storage and interval metering are both set: one table kind per engine',
 'intervals, then storage': 'battery storage and interval metering are both set: one table kind per engine',
 'storage, then registers': 'battery storage and the import / export registers are both set: one table kind per engine',
 'registers, then storage': 'battery storage and the import / export registers are both set: one table kind per engine',
 'storage, then demand': 'battery storage and the demand registers are both set: one table kind per engine',
 'demand, then storage': 'battery storage and the demand registers are both set: one table kind per engine',
 'storage, then battery': 'the battery kind and battery storage are both set: one table kind per engine',
 'battery, then storage': 'the battery kind and battery storage are both set: one table kind per engine',
 'storage, then battery_sweep': 'the battery sweep and battery storage are both set: one table kind per engine',
 'battery_sweep, then storage': 'the battery sweep and battery storage are both set: one table kind per engine',
 'storage, then dispatch': 'battery dispatch and battery storage are both set: one table kind per engine',
 'dispatch, then storage': 'battery dispatch and battery storage are both set: one table kind per engine',
 'storage, then dispatch_sweep': 'the dispatch sweep and battery storage are both set: one table kind per engine',
 'dispatch_sweep, then storage': 'the dispatch sweep and battery storage are both set: one table kind per engine',
 'storage, then schedule': 'the schedule and battery storage are both set: one table kind per engine',
 'schedule, then storage': 'the schedule and battery storage are both set: one table kind per engine',
 'storage beside a series': 'storage tables and a fleet series are both set: one of the two per engine',
 'storage beside a battery_fleet': 'a battery fleet series cannot run beside battery storage (tmh_set_storage, the lossless kind): use the battery '
                                   'kind with efficiencies 1',
 'storage with per-chain sites': None,
 'storage, work buffer one byte short': 'storage tables work buffer too small for this window: 3071 < 3072',
 'battery, then intervals': 'the battery kind and interval metering are both set: one table kind per engine',
 'intervals, then battery': 'the battery kind and interval metering are both set: one table kind per engine',
 'battery, then registers': 'the battery kind and the import / export registers are both set: one table kind per engine',
 'registers, then battery': 'the battery kind and the import / export registers are both set: one table kind per engine',
 'battery, then demand': 'the battery kind and the demand registers are both set: one table kind per engine',
 'demand, then battery': 'the battery kind and the demand registers are both set: one table kind per engine',
 'battery, then battery_sweep': 'the battery sweep and the battery kind are both set: one table kind per engine',
 'battery_sweep, then battery': 'the battery sweep and the battery kind are both set: one table kind per engine',
 'battery, then dispatch': 'battery dispatch and the battery kind are both set: one table kind per engine',
 'dispatch, then battery': 'battery dispatch and the battery kind are both set: one table kind per engine',
 'battery, then dispatch_sweep': 'the dispatch sweep and the battery kind are both set: one table kind per engine',
 'dispatch_sweep, then battery': 'the dispatch sweep and the battery kind are both set: one table kind per engine',
 'battery, then schedule': 'the schedule and the battery kind are both set: one table kind per engine',
 'schedule, then battery': 'the schedule and the battery kind are both set: one table kind per engine',
 'battery beside a series': 'battery tables and a fleet series are both set: one of the two per engine',
 'battery beside a battery_fleet': None,
 'battery with per-chain sites': None,
 'battery, work buffer one byte short': 'battery tables work buffer too small for this window: 3071 < 3072',
 'battery_sweep, then intervals': 'the battery sweep and interval metering are both set: one table kind per engine',
 'intervals, then battery_sweep': 'the battery sweep and interval metering are both set: one table kind per engine',
 'battery_sweep, then registers': 'the battery sweep and the import / export registers are both set: one table kind per engine',
 'registers, then battery_sweep': 'the battery sweep and the import / export registers are both set: one table kind per engine',
 'battery_sweep, then demand': 'the battery sweep and the demand registers are both set: one table kind per engine',
 'demand, then battery_sweep': 'the battery sweep and the demand registers are both set: one table kind per engine',
 'battery_sweep, then dispatch': 'battery dispatch and the battery sweep are both set: one table kind per engine',
 'dispatch, then battery_sweep': 'battery dispatch and the battery sweep are both set: one table kind per engine',
 'battery_sweep, then dispatch_sweep': 'the dispatch sweep and the battery sweep are both set: one table kind per engine',
 'dispatch_sweep, then battery_sweep': 'the dispatch sweep and the battery sweep are both set: one table kind per engine',
 'battery_sweep, then schedule': 'the schedule and the battery sweep are both set: one table kind per engine',
 'schedule, then battery_sweep': 'the schedule and the battery sweep are both set: one table kind per engine',
 'battery_sweep beside a series': 'battery sweep tables and a fleet series are both set: one of the two per engine',
 'battery_sweep beside a battery_fleet': "the battery sweep and a battery fleet series are both set: the fleet series is the battery kind's (one "
                                         'battery per chain)',
 'battery_sweep with per-chain sites': 'the battery sweep cannot run with per-chain sites (tmh_set_sites)',
 'battery_sweep, work buffer one byte short': 'battery sweep tables work buffer too small for this window: 6143 < 6144',
 'dispatch, then intervals': 'battery dispatch and interval metering are both set: one table kind per engine',
 'intervals, then dispatch': 'battery dispatch and interval metering are both set: one table kind per engine',
 'dispatch, then registers': 'battery dispatch and the import / export registers are both set: one table kind per engine',
 'registers, then dispatch': 'battery dispatch and the import / export registers are both set: one table kind per engine',
 'dispatch, then demand': 'battery dispatch and the demand registers are both set: one table kind per engine',
 'demand, then dispatch': 'battery dispatch and the demand registers are both set: one table kind per engine',
 'dispatch, then dispatch_sweep': 'the dispatch sweep and battery dispatch are both set: one table kind per engine',
 'dispatch_sweep, then dispatch': 'the dispatch sweep and battery dispatch are both set: one table kind per engine',
 'dispatch, then schedule': 'the schedule and battery dispatch are both set: one table kind per engine',
 'schedule, then dispatch': 'the schedule and battery dispatch are both set: one table kind per engine',
 'dispatch beside a series': 'battery dispatch tables and a fleet series are both set: one of the two per engine',
 'dispatch beside a battery_fleet': "battery dispatch and a battery fleet series are both set: the fleet series is the battery kind's",
 'dispatch with per-chain sites': None,
 'dispatch, work buffer one byte short': 'battery dispatch tables work buffer too small for this window: 3071 < 3072',
 'dispatch_sweep, then intervals': 'the dispatch sweep and interval metering are both set: one table kind per engine',
 'intervals, then dispatch_sweep': 'the dispatch sweep and interval metering are both set: one table kind per engine',
 'dispatch_sweep, then registers': 'the dispatch sweep and the import / export registers are both set: one table kind per engine',
 'registers, then dispatch_sweep': 'the dispatch sweep and the import / export registers are both set: one table kind per engine',
 'dispatch_sweep, then demand': 'the dispatch sweep and the demand registers are both set: one table kind per engine',
 'demand, then dispatch_sweep': 'the dispatch sweep and the demand registers are both set: one table kind per engine',
 'dispatch_sweep, then schedule': 'the schedule and the dispatch sweep are both set: one table kind per engine',
 'schedule, then dispatch_sweep': 'the schedule and the dispatch sweep are both set: one table kind per engine',
 'dispatch_sweep beside a series': 'dispatch sweep tables and a fleet series are both set: one of the two per engine',
 'dispatch_sweep beside a battery_fleet': "the dispatch sweep and a battery fleet series are both set: the fleet series is the battery kind's (one "
                                          'battery per chain)',
 'dispatch_sweep with per-chain sites': 'the dispatch sweep cannot run with per-chain sites (tmh_set_sites)',
 'dispatch_sweep, work buffer one byte short': 'dispatch sweep tables work buffer too small for this window: 6143 < 6144',
 'schedule, then intervals': 'the schedule and interval metering are both set: one table kind per engine',
 'intervals, then schedule': 'the schedule and interval metering are both set: one table kind per engine',
 'schedule, then registers': 'the schedule and the import / export registers are both set: one table kind per engine',
 'registers, then schedule': 'the schedule and the import / export registers are both set: one table kind per engine',
 'schedule, then demand': 'the schedule and the demand registers are both set: one table kind per engine',
 'demand, then schedule': 'the schedule and the demand registers are both set: one table kind per engine',
 'schedule beside a series': 'schedule tables and a fleet series are both set: one of the two per engine',
 'schedule beside a battery_fleet': "the schedule and a battery fleet series are both set: the fleet series is the battery kind's",
 'schedule with per-chain sites': 'the schedule cannot run with per-chain sites (tmh_set_sites)',
 'schedule, work buffer one byte short': 'schedule tables work buffer too small for this window: 3071 < 3072'}


def test_refusal_precedence_word_for_word():
    got = _refusals()
    assert len(got) == 66 + 24
    assert got == EXPECTED


QUANTITIES = dict(capacity_wh=0.5, charge_w=1000.0, discharge_w=3000.0, soc0_wh=0.25)
SWEEP = dict(capacity_wh=[0.5, 0.2], soc0_wh=[0.25, 0.1])
LOSSES = dict(charge_eff=0.95, discharge_eff=0.9, standby_w=2.0)
RULE = dict(charge_above_w=50.0, discharge_above_w=100.0, feed_in_limit_w=2000.0)
ARGS = {
    "storage": QUANTITIES,
    "battery": dict(QUANTITIES, **LOSSES),
    "dispatch": dict(QUANTITIES, **LOSSES, **RULE),
    "schedule": dict(QUANTITIES, **LOSSES, rules=[dict(RULE, grid_charge_w=0.0), dict(RULE, grid_charge_w=500.0)]),
    "battery_sweep": {**QUANTITIES, **LOSSES, **SWEEP},
    "dispatch_sweep": {**QUANTITIES, **LOSSES, **RULE, **SWEEP},
}


def _fresh():
    return _sim(N, START, prec="fp64", mp=modules_params(), horizon=2 * 86400)


def _result(sim, kind):
    torch.cuda.synchronize()
    raw, soc = _np(getattr(sim, kind + "_raw")), _np(sim.soc)
    assert raw[..., 6, :].any() and raw[..., 7, :].any()   # (the batteries took and gave something)
    return raw, soc


@pytest.mark.parametrize("kind", ["storage", "battery", "dispatch", "schedule"])
def test_work_buffer_grows_with_the_window(kind):
    """Enabled for 100 steps and again for 1000, a sim keeps the work buffer of one block; run(1000) grows it
    (_work_window) and gives the bits of a sim enabled once."""
    def enable(sim, n_steps):
        more = dict(rule_of_interval=[k % 2 for k in range(-(-n_steps // IV))]) if kind == "schedule" else {}
        return getattr(sim, "enable_" + kind)(n_steps, IV, **ARGS[kind], **more)

    sim = _fresh()
    enable(sim, 100)
    small = sim._battery_work.numel()
    assert small == sim.L.tmh_storage_work_bytes(N, 100)
    enable(sim, 1000)
    assert sim._battery_work.numel() == small
    sim.run(1000, trace=())
    assert sim._battery_work.numel() == sim.L.tmh_storage_work_bytes(N, 1000) > small
    once = _fresh()
    enable(once, 1000)
    once.run(1000, trace=())
    for got, want in zip(_result(sim, kind), _result(once, kind)):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("kind", ["battery_sweep", "dispatch_sweep"])
def test_sweep_work_buffer_grows_with_the_window(kind):
    """A sweep's work buffer holds a day; one window of 86,528 steps grows it (_work_window) and gives the bits of
    two windows of 43,264."""
    steps, res = 86528, []
    for window in (steps, steps // 2):
        sim = _fresh()
        getattr(sim, "enable_" + kind)(steps, IV, **ARGS[kind])
        day = sim._battery_work.numel()
        assert day == sim.L.tmh_battery_sweep_work_bytes(N, 86400, 2)
        sim.run(steps, trace=(), window=window)
        assert (sim._battery_work.numel() > day) == (window == steps)
        res.append(_result(sim, kind))
    for got, want in zip(*res):
        np.testing.assert_array_equal(got, want)
