"""Ensembles behind the scoring server (GPU): one server with 5 models and one ensemble, two worker processes
(tests/serve_worker_ensemble.py, NumPy only) that send host states and LP snapshots under the ensemble's name and under a plain
model key, interleaved, through the existing kinds 0-5.

Every ensemble request is answered with its own call, so its reply must equal `ModelSet.*_ensemble` in this process bit for bit
(`np.array_equal`, no tolerance): the mean, the rankings, the selection and cut_index; the members never travel.  The plain
replies are what they were: their grouping depends on timing, so they are held against the model's own single call within the
1e-4 of tests/test_gpu_serve.py.  Half-way each worker opens a resident LP under the ensemble's name -- refused with the reply of
an unknown model -- and goes on."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

import serve_worker_ensemble as W  # noqa: E402
from gcnn_cut_selector_amd import serve  # noqa: E402
from gcnn_cut_selector_amd.model import ModelSet  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [f"setcov/{i}" for i in range(5)]
NAME, PLAIN = "setcov/ensemble", KEYS[3]
N_WORKERS = 2


def test_two_workers_under_an_ensemble_name_and_a_plain_key(dev, tmp_path):  # noqa: F811
    models = {k: make_model(700 + i, dev)[0] for i, k in enumerate(KEYS)}
    order = [KEYS[2], KEYS[0], KEYS[4], KEYS[1], KEYS[3]]          # the ensemble's own order, not the server's
    address = str(tmp_path / "gcnn.sock")
    with pytest.raises(ValueError):
        serve.ScoringServer(models, address, ensembles={PLAIN: order})
    server = serve.ScoringServer(models, address, ensembles={NAME: order})
    worker = os.path.join(ROOT, "tests", "serve_worker_ensemble.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), NAME, PLAIN,
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
    assert stats["requests"] == N_WORKERS * (W.N_REQUESTS + 1) and stats["errors"] == N_WORKERS
    assert stats["ensemble_calls"] == N_WORKERS * W.N_REQUESTS // 2 and stats["sessions_open"] == 0
    mset = ModelSet(models)
    plain = models[PLAIN]
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        assert "no model 'setcov/ensemble'" in bytes(got["refused"]).decode()
        for j in range(W.N_REQUESTS):
            ens, lp, kind, what, forced, (p_max, p_max_ub) = W.request(w, j)
            q = got[f"s{j}"]
            if kind == serve.KIND_SELECT:
                if ens:
                    select = mset.select_cuts_lp_ensemble if lp else mset.select_cuts_ensemble
                    want = select(order, what, forced, p_max=p_max, p_max_ub=p_max_ub, max_selected=W.MAX_SELECTED)
                else:
                    want = (plain.select_cuts_lp if lp else plain.select_cuts)(what, forced, p_max=p_max, p_max_ub=p_max_ub,
                                                                               max_selected=W.MAX_SELECTED)
                scores, index = np.asarray(want.scores), want.cut_index
                if ens:
                    assert np.array_equal(got[f"o{j}"], want.order) and int(got[f"n{j}"]) == want.n_kept, (w, j)
            else:
                if ens:
                    want = (mset.score_lp_ensemble if lp else mset.score_ensemble)(order, what, rank=kind == serve.KIND_RANK)
                else:
                    want = (plain.score_lp if lp else plain.score_state)(what, rank=kind == serve.KIND_RANK)
                scores, index = np.asarray(want), want.cut_index
                if kind == serve.KIND_RANK:
                    assert list(got[f"o{j}"]) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (w, j)
            assert q.dtype == np.float32 and q.shape == scores.shape, (w, j)
            if ens:
                assert q.tobytes() == scores.tobytes(), (w, j)                   # the mean, bit for bit
                assert want.members.shape == (5, q.shape[0])                     # (the members stayed in the server)
            else:
                np.testing.assert_allclose(q, scores, rtol=1e-4, atol=1e-4)
            if lp:
                assert np.array_equal(got[f"i{j}"], index), (w, j)
