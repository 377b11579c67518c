"""Expert rounds behind the scoring server (GPU): two torch-free workers play a data collector's rounds -- hybrid rounds and one expert
round each -- against a server that holds NO model, and get the in-process calls' bits; the worker that also sends a snapshot the
device rejects gets its error, and the other one is served."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import serve_worker_collect as W  # noqa: E402
from gcnn_cut_selector_amd import serve  # noqa: E402
from gcnn_cut_selector_amd.collect import Collector  # noqa: E402
from gcnn_cut_selector_amd.hybrid import HybridSelector  # noqa: E402

from gpucommon import dev  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WORKERS = 2


def test_two_collector_workers_against_a_server_without_a_model(dev, tmp_path):  # noqa: F811
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer({}, address).start()
    worker = os.path.join(ROOT, "tests", "serve_worker_collect.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), str(tmp_path / f"w{w}.npz"),
                               str(int(w == 0))]) for w in range(N_WORKERS)]
    try:
        codes = [p.wait(timeout=150) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * N_WORKERS
    # worker 0's bad snapshot is the one error; its short quality never reached the server
    assert server.stats["errors"] == 1 and server.stats["collect_calls"] == N_WORKERS + 1
    assert server.stats["requests"] == N_WORKERS * (W.N_HYBRID + 1) + 1
    col, hyb = Collector(dev), HybridSelector(dev)
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        for j in range(W.N_HYBRID):
            snap, forced, _ = W.round_of(w, j)
            direct = hyb.select_cuts(snap, forced, max_selected=4)
            assert np.array_equal(got[f"o{j}"], direct.order) and int(got[f"n{j}"]) == direct.n_kept
            assert got[f"q{j}"].dtype == np.float64 and np.array_equal(got[f"q{j}"], direct.scores)
        snap, forced, quality = W.round_of(w, W.N_HYBRID)
        direct = col.collect_lp(snap, quality, forced, max_selected=6)
        for name, a in zip(W.STATE_NAMES, direct.state[:7]):
            assert got[name].dtype == a.dtype and got[name].shape == a.shape and np.array_equal(got[name], a), name
        assert tuple(got["sizes"]) == direct.state[7:]
        assert np.array_equal(got["cut_index"], direct.cut_index) and not np.array_equal(direct.cut_index, np.arange(direct.cut_index.size))
        assert got["improvements"].dtype == np.float64 and np.array_equal(got["improvements"], quality[direct.cut_index])
        assert np.array_equal(got["order"], direct.order) and int(got["n_kept"]) == direct.n_kept < quality.size
        assert np.array_equal(got["hybrid_quality"], direct.hybrid_quality) and np.array_equal(got["features"], direct.features)
