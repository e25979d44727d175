"""The plain bench run on the GPU (`bench.py --gpus 1 --steps K --warmup W`): the headline alone.

It times K steps and prints one line with the contract fields and the roofline of its own timed
steps; the CPU baseline, parity, read peak, host-buffer rates, sweep, extras and latency block run
only with --full.  --dump-outputs writes the last timed step's root.  Small object: 64 MiB at
1 MiB chunks (64 leaves, BASELINE configs[0]'s bytes and seed stream), checked against the oracle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_common import SEED  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_run_is_the_headline_alone_and_dumps_its_root(oracle_lib, tmp_path):
    length, chunk, steps = 64 << 20, 1 << 20, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--object-gib", str(length / (1 << 30)), "--chunk", str(chunk),
                        "--dump-outputs", str(tmp_path / "dump"), "--detail-out", str(tmp_path / "d.json")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1                                  # no legs: the headline line, once
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 1 and line["unit"] == "GiB/s" and line["dtype"] == "u32"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0 and line["ok"] is True
    assert line["value"] == pytest.approx(length / (1 << 30) / (line["ms_per_step"] * 1e-3), rel=1e-2)
    rf = line["roofline"]
    assert rf["k1_launches"] == steps and rf["k1_avg_ms"] > 0      # the timed steps' own events, nothing run again
    assert "measured_read_peak_GBps" not in rf
    for k in ("cpu_baseline", "parity", "e2e", "sweep_gibs", "extras", "latency", "vs_cpu_share"):
        assert k not in line, k                             # all of that is --full
    _, want = oracle_lib.root_buffer(oracle_lib.splitmix_bytes(length, SEED), chunk, nthreads=4)
    assert line["root"] == want.hex()
    a = np.load(tmp_path / "dump" / "root.npy")
    assert a.dtype == np.float32 and bytes(a.astype(np.uint8)) == want
