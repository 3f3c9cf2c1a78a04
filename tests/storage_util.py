"""Shared by the battery-storage tests: the PV system "k modules" (test_gpu_registers.big_params' recipe with
factor k), the batteries of the main and the boundary tests in the engine's integers, and the events a
storage test input must hold (clips at both bounds, seconds strictly inside, both power limits binding)."""
import dataclasses
import functools

import numpy as np

from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, a_params

MODULES = 60                                   # Paco 15,000 W, below TMH_SERIES_MAX_W
A_BATTERY = dict(capacity_wh=0.5, charge_w=1000.0, discharge_w=3000.0, soc0_wh=0.25)     # soc0: half
C_BATTERY = dict(capacity_wh=0.05, charge_w=300.0, discharge_w=2000.0, soc0_wh=0.025)


def modules_params(k=MODULES):
    """A's parameters with a k-module system: k x the PV against the same meter."""
    mp = a_params()
    mod, inv = dict(mp.module), dict(mp.inverter)
    mod["Impo"] *= k
    for key in ("Paco", "Pdco", "Pso", "Pnt"):
        inv[key] *= k
    inv["C0"] /= k
    return dataclasses.replace(mp, module=mod, inverter=inv)


def battery(spec):
    """from_traces' keyword arguments of a battery given in Wh and W."""
    from tmhpvsim_amd import storage
    cap, pc, pd, x0 = storage.quantize_params(**spec)
    return dict(capacity=cap, p_charge=pc, p_discharge=pd, soc0=x0)


@functools.lru_cache(maxsize=None)
def a60_oracle():
    """The oracle's fp64 traces of A with 60 modules: dict(pv, meter, covered [steps, n], status [n])."""
    from oracle import oracle as O
    ref = O.run(modules_params(), A_CHAIN0, A_N, A_STEPS, A_START, tz=A_TZ, n_threads=8,
                outputs=("covered", "pv", "meter"))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def events(pv, meter, cov, *, capacity, p_charge, p_discharge, soc0):
    """Counts over traces [steps, n] of what makes a battery input bite, from a plain sequential run:
    ok seconds clipped at full and at empty (the battery could not take / give all it was asked),
    ok seconds whose SoC is strictly inside (0, C) afterwards, seconds at which the charge and the
    discharge limit bind, and the chains that hit both bounds."""
    from tmhpvsim_amd import storage
    pv, meter, cov = (np.asarray(a) for a in (pv, meter, cov))
    ok = ~(np.isnan(pv) | np.isnan(meter) | (cov == 255))
    d = np.where(ok, storage.quantize(pv) - storage.quantize(meter), 0).astype(np.int64)
    a = np.clip(d, -p_discharge, p_charge)
    x = np.full(pv.shape[1], soc0, dtype=np.int64)
    full = empty = inside = 0
    hit_full, hit_empty = np.zeros(pv.shape[1], bool), np.zeros(pv.shape[1], bool)
    for s in range(pv.shape[0]):
        t = x + a[s]
        f, e = ok[s] & (t > capacity), ok[s] & (t < 0)
        x = np.where(ok[s], np.clip(t, 0, capacity), x)
        full += int(f.sum())
        empty += int(e.sum())
        inside += int((ok[s] & (x > 0) & (x < capacity)).sum())
        hit_full |= f
        hit_empty |= e
    return dict(full=full, empty=empty, inside=inside, charge_limit=int((ok & (d > p_charge)).sum()),
                discharge_limit=int((ok & (d < -p_discharge)).sum()), both=int((hit_full & hit_empty).sum()))
