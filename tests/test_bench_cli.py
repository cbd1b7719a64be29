"""bench.py's plain run: the headline line alone, --steps timed steps in all, --dump-outputs writing
the last timed step's per-job verdicts.  One slot per batch keeps each case to a few seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 3 steps over 7 engines (four engines run none), 9 over 7 (uneven split), one engine alone
@pytest.mark.gpu
@pytest.mark.parametrize("steps,inflight", [(3, 7), (9, 7), (2, 1)])
def test_plain_run_line_and_dump(tmp_path, steps, inflight):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--slots", "1", "--inflight", str(inflight), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == 1 and line["config"]["inflight"] == inflight
    assert line["unit"] == "sets/s" and line["higher_is_better"] is True and line["dtype"].startswith("u32")
    n_sets, n_jobs = line["config"]["sets_per_gpu"], line["config"]["jobs_per_gpu"]
    assert (n_sets, n_jobs) == (19456, 17408)
    # value and ms_per_step describe the same timed region of `steps` batch verifications
    assert line["value"] == pytest.approx(n_sets / (line["ms_per_step"] * 1e-3), rel=1e-3)
    # the secondary measurements belong to --full
    for k in ("roofline", "cpu_baseline", "value_one_batch_in_flight", "value_distinct_roots", "per_config",
              "range_sync_segments", "value_e2e", "value_dropin"):
        assert k not in line, k
    assert sorted(os.listdir(out)) == ["codes.npy"]
    codes = np.load(out / "codes.npy")
    assert codes.dtype == np.float32 and codes.shape == (n_jobs,)
    assert np.array_equal(codes, np.ones(n_jobs, np.float32))  # c3: every job valid
