"""Resident LPs behind the scoring server on the GPU: four torch-free worker processes (tests/serve_worker_lpsession.py) each
open an LP at the server and run three rounds with appends on it; every reply equals the in-process solo `LPSession`'s, bit for
bit, and the sessions are gone once the workers have left.  (How many rounds share a call depends on timing: the grouping itself
is tested on the CPU, tests/test_lprounds_host.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import serve_worker_lpsession as W  # noqa: E402
from gcnn_cut_selector_amd import serve  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WORKERS = 4


def test_workers_keep_their_lps_at_the_server(dev, tmp_path):  # noqa: F811
    models = {"m0": make_model(93, dev)[0], "m1": make_model(17, dev)[0]}
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer(models, address)      # bound and listening from here on: the workers' requests wait for start()
    worker = os.path.join(ROOT, "tests", "serve_worker_lpsession.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), str(tmp_path / f"w{w}.npz")])
             for w in range(N_WORKERS)]
    try:
        server.start()
        codes = [p.wait(timeout=150) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * N_WORKERS
    stats = server.stats
    assert stats["session_rounds"] == N_WORKERS * W.N_ROUNDS == 12 and stats["sessions_open"] == 0 and not server._sessions
    assert stats["errors"] == N_WORKERS and 1 <= stats["session_calls"] <= 12 and 1 <= stats["max_sessions_per_call"] <= N_WORKERS
    assert stats["requests"] == N_WORKERS * (W.N_ROUNDS + 3)          # open, the rounds, the foreign close, close
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        rows, rng, base, pools = W.script(w)
        sess = models[f"m{w % 2}"].open_lp(rows)
        want = W.play(w, sess, rows, rng, base, pools)
        sess.close()
        assert sorted(got.files) == sorted(want)
        for name, a in want.items():
            assert got[name].dtype == np.asarray(a).dtype and np.array_equal(got[name], a, equal_nan=True), (w, name)
