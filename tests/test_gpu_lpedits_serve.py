"""Removals through the scoring server on the GPU: four torch-free worker processes (tests/serve_worker_lpedits.py) each open an
LP at the server and run three rounds on it, every one of which carries an append and a removal; every reply equals the
in-process solo `LPSession`'s, bit for bit.  The server's loop is driven from the test in lock step -- a turn is served once
every connected worker has its request waiting (a worker has one request in flight at a time) -- so the four rounds of a step
share one call whatever the timing: no round goes solo, a call serves four sessions, and the session of the worker that leaves
without a close request goes with its connection."""
import os
import selectors
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import serve_worker_lpedits as W  # noqa: E402
from gcnn_cut_selector_amd import serve  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WORKERS = 4


def _lock_step(server, procs, deadline):
    """`serve_forever`, except that what has arrived is served only once every open connection has a request waiting, and not
    before all workers have connected.  Ends when every worker has left."""
    server._sel = sel = selectors.DefaultSelector()
    sel.register(server._listen, selectors.EVENT_READ)
    pending, connected, turns = [], 0, []
    while connected < N_WORKERS or server._buffers:
        assert time.monotonic() < deadline, "the workers did not finish"
        assert not [p.returncode for p in procs if p.poll()], "a worker failed"
        for key, _ in sel.select(1.0):
            s = key.fileobj
            if s is server._listen:
                server._accept()
                connected += 1
            else:
                server._read(s, pending)
        pending = [(c, r) for c, r in pending if c in server._buffers]
        if connected == N_WORKERS and pending and {c for c, _ in pending} == set(server._buffers):
            batch, pending = pending, []
            turns.append(sorted({r["kind"] for _, r in batch}))
            server._serve(batch)
    sel.close()
    return turns


def test_workers_append_and_remove_through_the_server(dev, tmp_path):  # noqa: F811
    models = {"m0": make_model(93, dev)[0], "m1": make_model(17, dev)[0]}
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer(models, address)      # bound and listening from here on
    worker = os.path.join(ROOT, "tests", "serve_worker_lpedits.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), str(tmp_path / f"w{w}.npz")])
             for w in range(N_WORKERS)]
    try:
        turns = _lock_step(server, procs, time.monotonic() + 120)
        codes = [p.wait(timeout=30) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server._shutdown()
    assert codes == [0] * N_WORKERS
    # open | three rounds of four | the removals alone of three workers | their closes
    assert turns == [[serve.KIND_LP_OPEN]] + [[serve.KIND_LP_ROUND]] * 4 + [[serve.KIND_LP_CLOSE]], turns
    stats = server.stats
    assert stats["session_rounds"] == N_WORKERS * W.N_ROUNDS == 12 and stats["session_calls"] == W.N_ROUNDS
    assert stats["session_solo_rounds"] == 0 and stats["max_sessions_per_call"] == N_WORKERS == 4
    assert stats["errors"] == 0 and stats["requests"] == N_WORKERS * (W.N_ROUNDS + 1) + 2 * (N_WORKERS - 1)
    assert stats["sessions_open"] == 0 and not server._sessions                 # the early leaver's session went with its connection
    assert server._session_group.batch_removes and server._session_group.solo_rounds == 0
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        rows, rng, base, pools = W.script(w)
        sess = models[f"m{w % 2}"].open_lp(rows)
        want = W.play(w, sess, rows, rng, base, pools)
        sess.close()
        assert sorted(got.files) == sorted(want)
        for name, a in want.items():
            assert got[name].dtype == np.asarray(a).dtype and np.array_equal(got[name], a, equal_nan=True), (w, name)
