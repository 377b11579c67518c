"""The scoring server (GPU): eight torch-free worker processes, two models, mixed kinds of requests; every reply against the direct
answer of the same model and against its own scores; grouping; bad requests; shutdown."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
from gcnn_cut_selector_amd import serve  # noqa: E402

import serve_worker_requests as W  # noqa: E402
from gpucommon import make_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WORKERS = 8


def test_server_with_eight_workers(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda", 0)
    models = {"a": make_model(98, dev)[0], "b": make_model(99, dev)[0]}
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer(models, address)
    assert os.path.exists(address)
    worker = os.path.join(ROOT, "tests", "serve_worker.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, worker, ROOT, address, str(w), str(tmp_path / f"w{w}.npz"),
                               str(tmp_path / f"ready{w}")]) for w in range(N_WORKERS)]
    try:
        # The workers connect to the listening socket and send their first request before the server serves: whether or not eight
        # clients ever overlap on this machine later on, the first sweep finds several requests waiting and must group them.
        deadline = time.time() + 120
        while not all(os.path.exists(tmp_path / f"ready{w}") for w in range(N_WORKERS)):
            assert time.time() < deadline and all(p.poll() is None for p in procs), "a worker did not get ready"
            time.sleep(0.05)
        time.sleep(0.5)
        assert server.stats["requests"] == 0
        server.start()
        codes = [p.wait(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * N_WORKERS
    assert not os.path.exists(address)                                     # close() removed the socket file
    stats = server.stats
    bad = 3 * (N_WORKERS // 2)
    assert stats["errors"] == bad and stats["requests"] == N_WORKERS * W.N_REQUESTS + (N_WORKERS // 2) * 8
    assert stats["batched_calls"] >= 1 and stats["max_batch"] >= 2, stats   # at least one call served more than one request
    assert stats["calls"] < stats["requests"] - bad
    # every reply: the direct answer of the same model within the fp64 bound's 1e-4, and a valid ranking / selection of its own scores
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        for j in range(W.N_REQUESTS):
            key, kind, state, (p_max, p_max_ub) = W.request(w, j)
            q = got[f"s{j}"]
            assert q.dtype == np.float32 and q.shape == (state[9],)
            if kind == serve.KIND_SELECT:
                direct = models[key].select_cuts(state, p_max=p_max, p_max_ub=p_max_ub)
                np.testing.assert_allclose(q, direct.scores.numpy(), rtol=1e-4, atol=1e-4)
                rec = {}
                order, n = R.select(q, R.dense_rows(state[5][0], state[5][1], state[6].reshape(-1), state[9], state[8]), None,
                                    p_max, p_max_ub, record=rec)
                assert R.margins_ok(rec, p_max, p_max_ub), (w, j)
                assert np.array_equal(got[f"o{j}"], order) and int(got[f"n{j}"]) == n, (w, j)
            else:
                np.testing.assert_allclose(q, models[key].score_state(state).numpy(), rtol=1e-4, atol=1e-4)
                if kind == serve.KIND_RANK:
                    assert list(got[f"o{j}"]) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (w, j)
