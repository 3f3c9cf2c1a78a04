"""Base input A of the fleet-series tests and its oracle traces (computed once per
process, never modified): markov cloud cover, 1,000 chains from 5000, from 05:30 local
over 10,803 steps (no multiple of 4 or 128) -- chains faulted at construction, chains
that fault inside the window, night and daylight."""
import functools

import numpy as np

A_N, A_CHAIN0, A_STEPS = 1000, 5000, 10803
A_START, A_TZ = "2019-09-05 05:30:00", "Europe/Berlin"
A_WINDOWS = (5001, 5802)   # the second window starts off the four-step grid


def a_params():
    from tmhpvsim_amd.params import CC_MARKOV, ModelParams
    return ModelParams(cc_mode=CC_MARKOV)


@functools.lru_cache(maxsize=None)
def a_oracle():
    """The oracle's fp64 traces of A: dict(pv, meter, covered [steps, n], status [n])."""
    from oracle import oracle as O
    ref = O.run(a_params(), A_CHAIN0, A_N, A_STEPS, A_START, tz=A_TZ, n_threads=8,
                outputs=("covered", "pv", "meter"))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def a_has_teeth(pv, covered, status):
    """What every test on A asserts of its input (traces [steps, n] as numpy; NaN / 255 after a
    fault): at least 3 faults inside the window, at least 10 at construction, and a first
    daylight step inside the window.  Returns (in-window fault steps, first daylight step)."""
    pv, covered, status = np.asarray(pv), np.asarray(covered), np.asarray(status)
    born_dead = status == 1
    assert int(born_dead.sum()) >= 10, int(born_dead.sum())
    bad = covered == 255
    assert bad[:, born_dead].all()
    faulted = bad[-1] & ~bad[0]
    steps = np.sort(np.argmax(bad[:, faulted], axis=0))
    assert len(steps) >= 3, steps
    day = np.nan_to_num(pv, nan=0.0).max(axis=1) > 0
    first = int(np.argmax(day))
    assert day.any() and 0 < first < pv.shape[0] - 1, first
    return steps, first
