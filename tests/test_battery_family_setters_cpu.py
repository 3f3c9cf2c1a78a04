"""The six battery-family setters (tmh_set_storage, tmh_set_battery, tmh_set_battery_sweep, tmh_set_dispatch,
tmh_set_dispatch_sweep, tmh_set_schedule) share one host path; every refusal keeps its words.  Each bad field of
each setter's struct, called with a NULL engine (the struct is checked first), gives exactly the text below."""
import ctypes as C

import numpy as np
import pytest

from tmhpvsim_amd import _lib

# per kind: the ctypes struct, the fields after soc / work / work_bytes of a good struct, the count field with its
# maximum (None: the kind has no count), and whether the setter has a floor on work_bytes (one block of one chain per
# variant: 24 bytes)
KINDS = {
    "storage": (_lib.Storage, dict(capacity=1000, p_charge=10, p_discharge=10), None, False),
    "battery": (_lib.Battery, dict(params=True), None, False),
    "battery_sweep": (_lib.BatterySweep, dict(params=True, n_variants=2), ("n_variants", 16), True),
    "dispatch": (_lib.Dispatch, dict(params=True), None, False),
    "dispatch_sweep": (_lib.DispatchSweep, dict(params=True, n_variants=2), ("n_variants", 16), True),
    "schedule": (_lib.Schedule, dict(params=True, rule_of_interval=True, n_rules=2), ("n_rules", 8), True),
}


def cases(kind, addr):
    """(label, struct) of every bad field of kind's struct and of the good one; addr: an 8-byte aligned address."""
    cls, extra, count, floor = KINDS[kind]
    table = dict(sum=addr, step0=0, n_steps=10, interval_s=10, ld=4)
    good = dict(soc=addr, work=addr, work_bytes=24 * extra.get("n_variants", 1),
                **{k: (addr if v is True else v) for k, v in extra.items()})
    bad = [("sum NULL", dict(sum=None), {}), ("sum misaligned", dict(sum=addr + 4), {}), ("n_steps 0", dict(n_steps=0), {}),
           ("ld 0", dict(ld=0), {}), ("interval_s 0", dict(interval_s=0), {}), ("interval_s 2^23", dict(interval_s=1 << 23), {})]
    for f in ("soc", "work") + (("params",) if "params" in extra else ()):
        bad += [(f + " NULL", {}, {f: None}), (f + " misaligned", {}, {f: addr + 4})]
    if count:
        bad += [(count[0] + " 0", {}, {count[0]: 0}), (count[0] + " max + 1", {}, {count[0]: count[1] + 1})]
    if floor:
        bad.append(("work_bytes floor - 1", {}, dict(work_bytes=good["work_bytes"] - 1)))
    if kind == "storage":
        bad += [("capacity -1", {}, dict(capacity=-1)), ("capacity 2^40", {}, dict(capacity=1 << 40)),
                ("p_charge -1", {}, dict(p_charge=-1)), ("p_charge 2^27 + 1", {}, dict(p_charge=(1 << 27) + 1)),
                ("p_discharge -1", {}, dict(p_discharge=-1)), ("p_discharge 2^27 + 1", {}, dict(p_discharge=(1 << 27) + 1))]
    if kind == "schedule":
        bad.append(("rule_of_interval NULL", {}, dict(rule_of_interval=None)))
    bad.append(("good", {}, {}))
    for label, tkw, kw in bad:
        yield label, cls(table=_lib.Intervals(**{**table, **tkw}), **{**good, **kw})


# tmh_last_error() of the library built from commit d967865 (before the six setters became one), case by case
EXPECTED = {'storage': {'sum NULL': 'storage tables need a buffer, n_steps > 0 and ld > 0',
             'sum misaligned': 'storage tables buffer must be 8-byte aligned',
             'n_steps 0': 'storage tables need a buffer, n_steps > 0 and ld > 0',
             'ld 0': 'storage tables need a buffer, n_steps > 0 and ld > 0',
             'interval_s 0': 'storage tables: interval_s must be >= 1',
             'interval_s 2^23': "storage tables: interval_s 8388608 > 2^23 - 1 (the SoC key holds the second's offset above 40 bits)",
             'soc NULL': 'storage tables need an 8-byte aligned soc buffer',
             'soc misaligned': 'storage tables need an 8-byte aligned soc buffer',
             'work NULL': 'storage tables need an 8-byte aligned work buffer',
             'work misaligned': 'storage tables need an 8-byte aligned work buffer',
             'capacity -1': 'storage tables: capacity -1 outside [0, 2^40)',
             'capacity 2^40': 'storage tables: capacity 1099511627776 outside [0, 2^40)',
             'p_charge -1': 'storage tables: p_charge -1, p_discharge 10 outside [0, 2^27]',
             'p_charge 2^27 + 1': 'storage tables: p_charge 134217729, p_discharge 10 outside [0, 2^27]',
             'p_discharge -1': 'storage tables: p_charge 10, p_discharge -1 outside [0, 2^27]',
             'p_discharge 2^27 + 1': 'storage tables: p_charge 10, p_discharge 134217729 outside [0, 2^27]',
             'good': 'NULL engine'},
 'battery': {'sum NULL': 'battery tables need a buffer, n_steps > 0 and ld > 0',
             'sum misaligned': 'battery tables buffer must be 8-byte aligned',
             'n_steps 0': 'battery tables need a buffer, n_steps > 0 and ld > 0',
             'ld 0': 'battery tables need a buffer, n_steps > 0 and ld > 0',
             'interval_s 0': 'battery tables: interval_s must be >= 1',
             'interval_s 2^23': "battery tables: interval_s 8388608 > 2^23 - 1 (the SoC key holds the second's offset above 40 bits)",
             'soc NULL': 'battery tables need an 8-byte aligned soc buffer',
             'soc misaligned': 'battery tables need an 8-byte aligned soc buffer',
             'work NULL': 'battery tables need an 8-byte aligned work buffer',
             'work misaligned': 'battery tables need an 8-byte aligned work buffer',
             'params NULL': 'battery tables need an 8-byte aligned params tensor [6][ld]',
             'params misaligned': 'battery tables need an 8-byte aligned params tensor [6][ld]',
             'good': 'NULL engine'},
 'battery_sweep': {'sum NULL': 'battery sweep tables need a buffer, n_steps > 0 and ld > 0',
                   'sum misaligned': 'battery sweep tables buffer must be 8-byte aligned',
                   'n_steps 0': 'battery sweep tables need a buffer, n_steps > 0 and ld > 0',
                   'ld 0': 'battery sweep tables need a buffer, n_steps > 0 and ld > 0',
                   'interval_s 0': 'battery sweep tables: interval_s must be >= 1',
                   'interval_s 2^23': "battery sweep tables: interval_s 8388608 > 2^23 - 1 (the SoC key holds the second's offset above 40 bits)",
                   'soc NULL': 'battery sweep tables need an 8-byte aligned soc buffer [n_variants][ld]',
                   'soc misaligned': 'battery sweep tables need an 8-byte aligned soc buffer [n_variants][ld]',
                   'work NULL': 'battery sweep tables need an 8-byte aligned work buffer',
                   'work misaligned': 'battery sweep tables need an 8-byte aligned work buffer',
                   'params NULL': 'battery sweep tables need an 8-byte aligned params tensor [n_variants][6][ld]',
                   'params misaligned': 'battery sweep tables need an 8-byte aligned params tensor [n_variants][6][ld]',
                   'n_variants 0': 'battery sweep tables: n_variants 0 outside [1, 16]',
                   'n_variants max + 1': 'battery sweep tables: n_variants 17 outside [1, 16]',
                   'work_bytes floor - 1': 'battery sweep tables work buffer too small: 47 < 48',
                   'good': 'NULL engine'},
 'dispatch': {'sum NULL': 'battery dispatch tables need a buffer, n_steps > 0 and ld > 0',
              'sum misaligned': 'battery dispatch tables buffer must be 8-byte aligned',
              'n_steps 0': 'battery dispatch tables need a buffer, n_steps > 0 and ld > 0',
              'ld 0': 'battery dispatch tables need a buffer, n_steps > 0 and ld > 0',
              'interval_s 0': 'battery dispatch tables: interval_s must be >= 1',
              'interval_s 2^23': "battery dispatch tables: interval_s 8388608 > 2^23 - 1 (the SoC key holds the second's offset above 40 bits)",
              'soc NULL': 'battery dispatch tables need an 8-byte aligned soc buffer',
              'soc misaligned': 'battery dispatch tables need an 8-byte aligned soc buffer',
              'work NULL': 'battery dispatch tables need an 8-byte aligned work buffer',
              'work misaligned': 'battery dispatch tables need an 8-byte aligned work buffer',
              'params NULL': 'battery dispatch tables need an 8-byte aligned params tensor [9][ld]',
              'params misaligned': 'battery dispatch tables need an 8-byte aligned params tensor [9][ld]',
              'good': 'NULL engine'},
 'dispatch_sweep': {'sum NULL': 'dispatch sweep tables need a buffer, n_steps > 0 and ld > 0',
                    'sum misaligned': 'dispatch sweep tables buffer must be 8-byte aligned',
                    'n_steps 0': 'dispatch sweep tables need a buffer, n_steps > 0 and ld > 0',
                    'ld 0': 'dispatch sweep tables need a buffer, n_steps > 0 and ld > 0',
                    'interval_s 0': 'dispatch sweep tables: interval_s must be >= 1',
                    'interval_s 2^23': "dispatch sweep tables: interval_s 8388608 > 2^23 - 1 (the SoC key holds the second's offset above 40 bits)",
                    'soc NULL': 'dispatch sweep tables need an 8-byte aligned soc buffer [n_variants][ld]',
                    'soc misaligned': 'dispatch sweep tables need an 8-byte aligned soc buffer [n_variants][ld]',
                    'work NULL': 'dispatch sweep tables need an 8-byte aligned work buffer',
                    'work misaligned': 'dispatch sweep tables need an 8-byte aligned work buffer',
                    'params NULL': 'dispatch sweep tables need an 8-byte aligned params tensor [n_variants][9][ld]',
                    'params misaligned': 'dispatch sweep tables need an 8-byte aligned params tensor [n_variants][9][ld]',
                    'n_variants 0': 'dispatch sweep tables: n_variants 0 outside [1, 16]',
                    'n_variants max + 1': 'dispatch sweep tables: n_variants 17 outside [1, 16]',
                    'work_bytes floor - 1': 'dispatch sweep tables work buffer too small: 47 < 48',
                    'good': 'NULL engine'},
 'schedule': {'sum NULL': 'schedule tables need a buffer, n_steps > 0 and ld > 0',
              'sum misaligned': 'schedule tables buffer must be 8-byte aligned',
              'n_steps 0': 'schedule tables need a buffer, n_steps > 0 and ld > 0',
              'ld 0': 'schedule tables need a buffer, n_steps > 0 and ld > 0',
              'interval_s 0': 'schedule tables: interval_s must be >= 1',
              'interval_s 2^23': "schedule tables: interval_s 8388608 > 2^23 - 1 (the SoC key holds the second's offset above 40 bits)",
              'soc NULL': 'schedule tables need an 8-byte aligned soc buffer',
              'soc misaligned': 'schedule tables need an 8-byte aligned soc buffer',
              'work NULL': 'schedule tables need an 8-byte aligned work buffer',
              'work misaligned': 'schedule tables need an 8-byte aligned work buffer',
              'params NULL': 'schedule tables need an 8-byte aligned params tensor [6 + 4 * n_rules][ld]',
              'params misaligned': 'schedule tables need an 8-byte aligned params tensor [6 + 4 * n_rules][ld]',
              'n_rules 0': 'schedule tables: n_rules 0 outside [1, 8]',
              'n_rules max + 1': 'schedule tables: n_rules 9 outside [1, 8]',
              'work_bytes floor - 1': 'schedule tables work buffer too small: 23 < 24',
              'rule_of_interval NULL': "schedule tables need a rule_of_interval array [n_intervals] (the schedule: each interval's rule)",
              'good': 'NULL engine'}}


@pytest.mark.parametrize("kind", list(KINDS))
def test_setter_refusals_word_for_word(kind):
    L = _lib.load()
    setter = getattr(L, "tmh_set_" + kind)
    buf = np.zeros(64, dtype=np.int64)
    got = {}
    for label, st in cases(kind, buf.ctypes.data):
        assert setter(None, C.byref(st)) == -1, (kind, label)
        got[label] = L.tmh_last_error().decode()
    assert setter(None, None) == -1 and L.tmh_last_error() == b"NULL engine"
    assert got == EXPECTED[kind]
