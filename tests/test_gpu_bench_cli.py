"""bench.py's command line on the GPU: a plain run prints the headline line only, --steps sets
the timed steps, and --dump-outputs writes the last timed step's results, which are the
oracle's for the same seeded workload (so the inputs do not change from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pyoracle import OracleScheduler
from tests.helpers import Case, run_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, BATCH, STEPS, WARMUP = 600, 150, 2, 1


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--nodes", str(NODES), "--batch", str(BATCH),
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "pods scheduled/sec" and d["unit"] == "pods/s" and d["higher_is_better"] is True
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(BATCH / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert d["config"]["timed_pods"] == [WARMUP * BATCH, (WARMUP + STEPS) * BATCH]
    # (what --full adds is not measured in a plain run)
    assert not {"roofline", "filter_score", "latency", "cpu_baseline"} & set(d)

    case = Case("config2", n_nodes=NODES, n_pods=(WARMUP + STEPS) * BATCH)
    orc = OracleScheduler(case.cfg)
    want, rng = run_batch(orc, case, chunk=BATCH)
    orc.close()
    assert sorted(os.listdir(tmp_path / "dump")) == ["placements.npy", "rng_state.npy"]
    got = np.load(tmp_path / "dump" / "placements.npy")
    st = np.load(tmp_path / "dump" / "rng_state.npy")
    assert got.dtype == np.float64 and st.dtype == np.float64
    assert np.array_equal(got, want[-BATCH:].astype(np.float64))
    assert (int(st[0]) << 32) | int(st[1]) == rng
