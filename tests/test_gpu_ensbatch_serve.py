"""Ensemble requests grouped behind the scoring server (GPU): one server with 5 models, one ensemble and `ensemble_batching=True`,
three worker processes (tests/serve_worker_ensbatch.py, NumPy only) that send host states and LP snapshots under the ensemble's
name through the kinds 1, 2, 4 and 5.

Which requests share a call depends on timing, and a state's bits depend on the union it rode in, so no reply is held against
another call bit for bit: every reply's scores are held against the fp64 oracle of the five-model mean on the state alone at the
project's 1e-4, and its order against its OWN scores -- the stable ranking, or the restated selection.  The grouping itself is
asserted by the stub test in tests/test_ensbatch_build.py."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
import serve_worker_ensbatch as W  # noqa: E402
from gcnn_cut_selector_amd import serve  # noqa: E402

from gpucommon import dev, make_model, oracle_scores  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [f"setcov/{i}" for i in range(5)]
NAME = "setcov/ensemble"
N_WORKERS = 3


def test_three_workers_under_an_ensemble_name_with_batching(dev, tmp_path):  # noqa: F811
    made = {k: make_model(900 + i, dev) for i, k in enumerate(KEYS)}
    models = {k: m for k, (m, _) in made.items()}
    order = [KEYS[2], KEYS[0], KEYS[4], KEYS[1], KEYS[3]]          # the ensemble's own order, not the server's
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer(models, address, ensembles={NAME: order}, ensemble_batching=True)
    worker = os.path.join(ROOT, "tests", "serve_worker_ensbatch.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), NAME,
                               str(tmp_path / f"w{w}.npz"), str(tmp_path / f"ready{w}")]) for w in range(N_WORKERS)]
    try:
        deadline = time.time() + 100
        while not all(os.path.exists(tmp_path / f"ready{w}") for w in range(N_WORKERS)):
            assert time.time() < deadline and all(p.poll() is None for p in procs), "a worker did not get ready"
            time.sleep(0.02)
        server.start()
        codes = [p.wait(timeout=130) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * N_WORKERS
    stats = server.stats
    print("server stats:", stats)
    assert stats["requests"] == N_WORKERS * W.N_REQUESTS and stats["errors"] == 0
    assert 1 <= stats["ensemble_calls"] <= stats["requests"] and stats["max_ensemble_batch"] >= 1
    assert stats["ensemble_batched_calls"] <= stats["ensemble_calls"] and stats["max_ensemble_batch"] <= N_WORKERS
    first = models[KEYS[0]]
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        for j in range(W.N_REQUESTS):
            kind, what, forced = W.request(w, j)
            lp, base = kind in serve._LP_BASE, serve._LP_BASE.get(kind, kind)
            q = got[f"s{j}"]
            state = what
            if lp:
                state, index = first.state_from_lp(what)
                assert np.array_equal(got[f"i{j}"], index), (w, j)
            K, V = state[9], state[8]
            want = np.mean([oracle_scores(made[k][1], state) for k in order], axis=0)
            assert q.dtype == np.float32 and q.shape == (K,), (w, j)
            np.testing.assert_allclose(q, want, rtol=1e-4, atol=1e-4)
            if base == serve.KIND_RANK:
                assert list(got[f"o{j}"]) == sorted(range(K), key=lambda x: q[x], reverse=True), (w, j)
            else:
                frows = None if forced is None else R.dense_rows(forced[0][0], forced[0][1], forced[1], forced[2], V)
                rec = {}
                sel, n = R.select(q, R.dense_rows(state[5][0], state[5][1], state[6].reshape(-1), K, V), frows, *W.THRESHOLDS, record=rec)
                assert sorted(got[f"o{j}"].tolist()) == list(range(K)), (w, j)
                if R.margins_ok(rec, *W.THRESHOLDS):      # (a parallelism on a threshold is the restatement's to decline, not a failure)
                    assert np.array_equal(got[f"o{j}"], sel) and int(got[f"n{j}"]) == n, (w, j)
