"""A plain bench.py run end to end, and what `--dump-outputs` writes, against the oracle.

One small run (1,000 chains x 2 h, three timed steps after one warm-up step, no
pre-warm) in a child process, as the benchmark is started: its line carries the
headline figures and nothing of the full report, and the dumped pv / meter /
residual of the last timed batch (batch 3: global chains 3,000-3,999) agree with
the C oracle at the sampled seconds and chains within the fp32 parity bar of the
trace tests (1e-5, DESIGN.md scales).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tmhpvsim_amd.params import ModelParams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SECS, STEPS, WARMUP = 1000, 7200, 3, 1
START, TZ = "2019-09-05 00:00:00", "Europe/Berlin"   # bench.py's C2 start and clock
FIELDS = ("pv", "meter", "residual")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--chains", str(N), "--seconds", str(SECS), "--prewarm-ms", "0",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), out


def test_plain_line_has_the_headline_and_no_full_report(run):
    line, _ = run
    assert line["unit"] == "chain-seconds/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["prewarm_batches"] == 0
    assert line["ms_per_step"] > 0
    # value = the timed steps' chain-seconds over their wall time
    assert line["value"] == pytest.approx(N * SECS * STEPS / (line["ms_per_step"] * STEPS / 1e3), rel=1e-9)
    assert line["full"] is False and "cpu_baseline" not in line and "secondary" not in line
    assert line["roofline"]["alone"] is None and line["roofline"]["kernel_ms"] > 0
    assert line["faulted_chains"] is not None


def test_dumped_outputs_are_the_last_batch_vs_oracle(run):
    line, out = run
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert set(got) == set(FIELDS) | {"status", "sample_seconds", "sample_chains"} == set(line["dumped_outputs"])
    assert sum(a.nbytes for a in got.values()) <= 64_000_000
    chain0 = (WARMUP + STEPS - 1) * N                        # fresh global ids every batch
    ref = O.run(ModelParams(), chain0, N, SECS, START, tz=TZ, n_threads=16, outputs=FIELDS)
    chains, seconds = got["sample_chains"].astype(int), got["sample_seconds"].astype(int)
    assert np.array_equal(chains, np.arange(N)) and 0 < len(seconds) < SECS    # the seconds are sampled here
    np.testing.assert_array_equal(got["status"], ref["status"][chains].astype(np.float32))
    ok = ref["status"][chains] == 0
    assert ok.mean() > 0.99
    g = {f: got[f].astype(np.float64) for f in FIELDS}
    r = {f: ref[f][seconds][:, chains] for f in FIELDS}
    for f in FIELDS:
        assert got[f].dtype == np.float32 and got[f].shape == (len(seconds), len(chains))
        np.testing.assert_array_equal(np.isnan(g[f]), np.isnan(r[f]))
    scale = {"pv": np.abs(r["pv"]), "meter": np.abs(r["meter"]), "residual": np.abs(r["meter"]) + np.abs(r["pv"])}
    for f in FIELDS:
        err = np.abs(g[f] - r[f])[:, ok] / np.maximum(scale[f][:, ok], 1.0)
        assert err.max() <= 1e-5, (f, float(err.max()))
