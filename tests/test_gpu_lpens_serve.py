"""Resident LPs under an ensemble's name through the scoring server on the GPU (`ScoringServer(..., ensemble_sessions=True)`):
three torch-free worker processes (tests/serve_worker_lpens.py) each keep an LP at the server through eight rounds of the
separation loop with appends and removals -- two under the ensemble's name, one under a model key at the same time.  Every reply
equals, bit for bit, the in-process one-shot call on the assembled snapshot: `ModelSet.select_cuts_lp_ensemble` for the ensemble's
workers, `GCNN.select_cuts_lp` for the plain one.  The server's loop is driven from the test in lock step, as in
tests/test_gpu_lpedits_serve.py.  A server with the default refuses the open under an ensemble's name, as before."""
import os
import selectors
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import serve_worker_lpens as W  # noqa: E402
import servecommon  # noqa: E402
from gcnn_cut_selector_amd import lpstate, serve  # noqa: E402
from gcnn_cut_selector_amd.infer import LPEnsembleSession  # noqa: E402
from gcnn_cut_selector_amd.model import ModelSet  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [f"seed/{i}" for i in range(5)]
WORKER_KEYS = ("five", "five", KEYS[3])       # two workers under the ensemble's name, one under a model key
N_WORKERS = len(WORKER_KEYS)


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


class _Assembled:
    """`LPSession.select_cuts`'s signature over the one-shot call `select(snapshot, forced, **kw)`: it keeps the rows and the
    optional column arrays on the host and answers every round on the assembled snapshot."""

    def __init__(self, rows, select):
        self.rows, self.select, self.kept = rows, select, {}

    @property
    def n_rows(self):
        return np.asarray(self.rows.row_lhs).shape[0]

    def select_cuts(self, rnd, forced=None, *, append=None, remove=None, **kw):
        if append is not None:
            self.rows = lpstate.rows_with(self.rows, append)
        if remove is not None:
            self.rows = lpstate.rows_without(self.rows, remove)
        res = self.select(lpstate.assemble(self.rows, rnd, self.kept), forced, **kw)
        self.kept.update({n: getattr(rnd, n) for n in lpstate.OPTIONAL if getattr(rnd, n) is not None})
        return res


def test_workers_keep_resident_lps_under_an_ensembles_name(dev, tmp_path):  # noqa: F811
    models = {k: make_model(600 + i, dev)[0] for i, k in enumerate(KEYS)}
    mset = ModelSet(models)
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer(models, address, model_set=mset, ensembles={"five": KEYS}, ensemble_sessions=True)
    worker = os.path.join(ROOT, "tests", "serve_worker_lpens.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), key, str(tmp_path / f"w{w}.npz")])
             for w, key in enumerate(WORKER_KEYS)]
    opened = []
    try:
        open_ensemble = mset.open_lp_ensemble

        def spy(*a, **kw):
            opened.append(open_ensemble(*a, **kw))
            return opened[-1]
        mset.open_lp_ensemble = spy
        turns = _lock_step(server, procs, time.monotonic() + 120)
        codes = [p.wait(timeout=30) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server._shutdown()
    assert codes == [0] * N_WORKERS
    assert turns == [[serve.KIND_LP_OPEN]] + [[serve.KIND_LP_ROUND]] * W.N_ROUNDS + [[serve.KIND_LP_CLOSE]], turns
    assert len(opened) == 2 and all(isinstance(s, LPEnsembleSession) and s.calls == W.N_ROUNDS and s.closed for s in opened)
    stats = server.stats
    assert stats["session_rounds"] == N_WORKERS * W.N_ROUNDS and stats["ensemble_calls"] == 2 * W.N_ROUNDS
    # the plain session's rounds are the group's, one session a call; the ensemble's never reach it
    assert stats["session_calls"] + stats["session_solo_rounds"] == W.N_ROUNDS and stats["max_sessions_per_call"] <= 1
    assert stats["errors"] == 0 and stats["requests"] == N_WORKERS * (W.N_ROUNDS + 2)
    assert stats["sessions_open"] == 0 and not server._sessions and not server._ensemble_sids
    for w, key in enumerate(WORKER_KEYS):
        got = np.load(tmp_path / f"w{w}.npz")
        rows, rng, base, pools = W.script(w)
        if key == "five":
            ref = _Assembled(rows, lambda snap, forced, **kw: mset.select_cuts_lp_ensemble(KEYS, snap, forced, **kw))
        else:
            ref = _Assembled(rows, models[key].select_cuts_lp)
        want = W.play(w, ref, rows, rng, base, pools)
        assert sorted(got.files) == sorted(want)
        for name, a in want.items():
            assert got[name].dtype == np.asarray(a).dtype and np.array_equal(got[name], a, equal_nan=True), (w, name)


def test_the_default_server_refuses_the_open(dev, tmp_path):  # noqa: F811
    models = {k: make_model(600 + i, dev)[0] for i, k in enumerate(KEYS[:2])}
    server = servecommon.stub_server(tmp_path, models, ensembles={"two": KEYS[:2]})
    try:
        assert server.ensemble_sessions is False
        peer = servecommon.Peer(server)
        peer.send(serve.encode_open_request("two", lpstate.LPRows.from_snapshot(servecommon.snap())))
        servecommon.pump(server, [peer])
        with pytest.raises(serve.ServerError, match="no model 'two'"):
            peer.reply()
        assert server.stats["errors"] == 1 and not server._sessions
    finally:
        servecommon.shut(server)
