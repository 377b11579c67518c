"""bench.py on the GPU: a plain run prints the headline line and nothing it does not need; `--full` adds the launch count and
the rooflines after the timed steps without changing what those steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GCNN_FORCE_DP")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *args],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1                                                  # ONE JSON line on stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["timing"]["steps_timed"] == 3
    assert not {"roofline", "roofline_step", "cpu_baseline"} & set(plain)
    assert "library_launches_per_step" not in plain["config"] and "gpu_over_cpu" not in plain["config"]
    full = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert all(k in full for k in HEADLINE) and full["timing"]["steps_timed"] == 3
    assert full["config"]["library_launches_per_step"] > 0
    assert full["roofline"]["achieved"] > 0 and full["roofline_step"]["launches"]
    assert "cpu_baseline" not in full
    for name in ("loss", "scores", "grads", "params"):                    # the extras run after the dumped step
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert np.isfinite(a).all() and np.array_equal(a, b), name
