"""Many LP snapshots in one call (GPU): `GCNN.score_lps` / `select_cuts_lp_many` (gcnn_lp_batch) and the LP requests of the scoring
server.  Both sides of every comparison run the same arithmetic in the same order -- the batched launches run the solo kernels'
bodies with snapshot-local block indices, and behind them gcnn_infer_batch's run half is the one `score_states` uses -- so
everything is compared with np.array_equal and no tolerance: a built state against `state_from_lp` of that snapshot alone, scores
and orders against `score_states` / `select_cuts_many` on the built states IN THE SAME UNION (a state's score bits may depend on
its neighbours through the forward pass's dispatch choice; its built state may not).  Only the server test, whose grouping depends on
timing, compares scores with the in-process single call within the 1e-4 of tests/test_gpu_serve.py.

Snapshots are the seam cases of tests/lpcases.py and small `synthetic.make_lp_snapshot`s: the smallest shapes at which the
builder changes path."""
import dataclasses
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cutsel_restate as R  # noqa: E402
import lpcases  # noqa: E402
import serve_worker_lp as W  # noqa: E402
from gcnn_cut_selector_amd import _lib, lpstate, serve, synthetic  # noqa: E402

from gpucommon import dev, make_model  # noqa: E402,F401
from test_lpbatch_build import NAMES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = dict(p_max=0.1, p_max_ub=0.5, max_selected=5)


@pytest.fixture(scope="module")
def model(dev):  # noqa: F811
    return make_model(93, dev)[0]


def _snap(name):
    if name == "setcov-noinc":
        return synthetic.make_lp_snapshot("setcov", 3, scale=0.3, incumbent=False)
    return lpcases.snapshot(name)


UNION = ("rows257", "cuts513", "cols257", "rows1", "setcov-noinc", "cuts256", "rows600", "cuts1100")
_alone = {}


def _built_alone(model, name):
    """`state_from_lp` of the snapshot alone: computed once, shared, never written to."""
    if name not in _alone:
        _alone[name] = model.state_from_lp(_snap(name))
    return _alone[name]


def _same_state(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:7], b[:7]))


def _same_scores(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _forced_for(state, seed):
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(state[8], size=6, replace=False))
    return (np.stack([np.repeat([0, 1], 3), cols]).astype(np.int32), rng.standard_normal(6).astype(np.float32), 2)


def test_same_bits_as_solo(model):
    snaps = [_snap(n) for n in UNION]
    built = [_built_alone(model, n) for n in UNION]
    states = [b[0] for b in built]
    sess = model._sess("_lp_batch_session", _lib_session())
    calls = sess.calls
    got = model.score_lps(snaps, rank=True)
    assert sess.calls == calls + 1
    for name, have, (state, index), q in zip(UNION, sess.last_states(), built, got):
        assert _same_state(have, state), name
        assert np.array_equal(q.cut_index, index), name
    want = model.score_states(states, rank=True)
    for name, q, q0 in zip(UNION, got, want):
        assert _same_scores(q, q0) and np.array_equal(q.rankings, q0.rankings), name
    forced = [_forced_for(s, i) if i % 2 else None for i, s in enumerate(states)]
    for f in (None, forced):
        sel = model.select_cuts_lp_many(snaps, f, **SELECT)
        sel0 = model.select_cuts_many(states, f, **SELECT)
        for name, s, s0, (_, index) in zip(UNION, sel, sel0, built):
            assert np.array_equal(s.order, s0.order) and (s.n_kept, s.n_selected) == (s0.n_kept, s0.n_selected), name
            assert _same_scores(s.scores, s0.scores) and np.array_equal(s.cut_index, index), name


def _lib_session():
    from gcnn_cut_selector_amd.infer import _LPBatchSession
    return _LPBatchSession


def test_built_state_does_not_depend_on_position(model):
    target = _built_alone(model, "rows600")[0]
    sess = model._sess("_lp_batch_session", _lib_session())
    for union, at in ((("rows600", "cuts257", "cols255"), 0), (("cuts513", "rows600", "rows1"), 1), (("cols256", "rows255", "rows600"), 2)):
        model.score_lps([_snap(n) for n in union])
        assert _same_state(sess.last_states()[at], target), union


def test_zero_block_and_arena_are_reusable(model):
    from gcnn_cut_selector_amd.model import GCNN
    big = [_snap(n) for n in ("cuts1100", "rows600", "cuts513", "rows257")]
    small = [_snap(n) for n in ("rows1", "cuts255", "cols257")]
    model.score_lps(big, rank=True)
    again = model.score_lps(small, rank=True)
    fresh_model = GCNN(device=model.device)
    fresh_model.set_weights(model.get_weights())
    fresh = fresh_model.score_lps(small, rank=True)
    for a, b in zip(again, fresh):
        assert _same_scores(a, b) and np.array_equal(a.rankings, b.rankings) and np.array_equal(a.cut_index, b.cut_index)
    sel, sel_fresh = model.select_cuts_lp_many(small, **SELECT), fresh_model.select_cuts_lp_many(small, **SELECT)
    for a, b in zip(sel, sel_fresh):
        assert np.array_equal(a.order, b.order) and a.n_kept == b.n_kept


def _without_rows(snap):
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    return dataclasses.replace(snap, row_ptr=np.zeros(1, np.int32), row_col=z(np.int32), row_val=z(np.float64), row_lhs=z(np.float64),
                               row_rhs=z(np.float64), row_dual=z(np.float64), row_basis=z(np.int8))


def _without_cuts(snap):
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    return dataclasses.replace(snap, cut_ptr=np.zeros(1, np.int32), cut_col=z(np.int32), cut_val=z(np.float64), cut_lhs=z(np.float64),
                               cut_rhs=z(np.float64))


def test_counts_and_empty_kinds(model):
    sess = model._sess("_lp_batch_session", _lib_session())
    small = [synthetic.make_lp_snapshot("indset", i, scale=0.2, n_cuts=3 + i % 5) for i in range(65)]
    calls = sess.calls
    first = model.score_lps(small[:64])
    assert sess.calls == calls + 1
    more = model.score_lps(small)
    assert sess.calls == calls + 3
    again = model.score_lps(small[:64])
    for a, b in zip(first, again):
        assert _same_scores(a, b)
    # 65 snapshots: the first 64 ride in the same union as before, the last one in a union of its own
    for a, b in zip(first, more[:64]):
        assert _same_scores(a, b) and np.array_equal(a.cut_index, b.cut_index)
    assert _same_scores(more[64], model.score_lps([small[64]])[0])
    # R = 0 and K = 0 in a union
    base = _snap("cuts255")
    no_rows, no_cuts = _without_rows(base), _without_cuts(base)
    calls = sess.calls
    got = model.score_lps([_snap("rows1"), no_rows, no_cuts, base], rank=True)
    assert sess.calls == calls + 1
    state, index = model.state_from_lp(no_rows)
    assert state[7] == 0 and _same_state(sess.last_states()[1], state) and np.array_equal(got[1].cut_index, index)
    want = model.score_states([_built_alone(model, "rows1")[0], state, _built_alone(model, "cuts255")[0]], rank=True)
    for q, q0 in zip((got[0], got[1], got[3]), want):
        assert _same_scores(q, q0) and np.array_equal(q.rankings, q0.rankings)
    alone = model.score_lp(no_cuts, rank=True)
    assert got[2].shape == alone.shape == (0,) and np.array_equal(got[2].cut_index, alone.cut_index)


def test_no_variable_limit(model):
    wide = synthetic.make_lp_snapshot("indset", 3, scale=0.3, extra_cols=33000)
    sess = model._sess("_lp_batch_session", _lib_session())
    solo_calls = []
    plain = model.score_lp
    model.score_lp = lambda *a, **k: solo_calls.append(1) or plain(*a, **k)
    try:
        got = model.score_lps([_snap("rows1"), wide, _snap("cuts255")], rank=True)
    finally:
        del model.score_lp
    assert not solo_calls
    state, index = model.state_from_lp(wide)
    assert state[8] > 32768 and _same_state(sess.last_states()[1], state) and np.array_equal(got[1].cut_index, index)
    want = model.score_states([_built_alone(model, "rows1")[0], state, _built_alone(model, "cuts255")[0]], rank=True)
    for q, q0 in zip(got, want):
        assert _same_scores(q, q0) and np.array_equal(q.rankings, q0.rankings)


def test_declined_snapshot_is_served_in_place(model):
    names = ("rows1", "cuts4097", "cuts255")
    snaps = [_snap(n) for n in names]
    got = model.score_lps(snaps, rank=True)
    alone = model.score_lp(snaps[1], rank=True)
    assert _same_scores(got[1], alone) and np.array_equal(got[1].rankings, alone.rankings) and np.array_equal(got[1].cut_index, alone.cut_index)
    without = model.score_lps([snaps[0], snaps[2]], rank=True)
    for q, q0 in zip((got[0], got[2]), without):
        assert _same_scores(q, q0) and np.array_equal(q.rankings, q0.rankings)


@pytest.mark.parametrize("field,where,value,text", [
    ("cut_col", 0, 10 ** 6, "outside"),                # a column far out of range
    ("row_col", 1, 0, "strictly increasing"),          # the second entry of row 0 repeats / precedes the first
    ("cut_ptr", 1, 10 ** 7, "monotone"),               # an offset beyond the entries
])
def test_a_bad_snapshot_stays_alone(model, monkeypatch, field, where, value, text):
    """The upload of the middle snapshot is corrupted behind the host check (deep_check is off): its slot holds the ValueError, its
    neighbours' bits are those of a run without it."""
    good = [_snap("rows257"), synthetic.make_lp_snapshot("setcov", 2, scale=0.3), _snap("cuts257")]
    clean = model.score_lps(good, rank=True)
    clean_sel = model.select_cuts_lp_many(good, **SELECT)
    index = [n for n, _ in lpstate.FIELDS].index(field) + 1
    pack, calls = lpstate.pack_snapshot, []

    def wrapper(buf, snap_off, arrays):
        pack(buf, snap_off, arrays)
        calls.append(1)
        if len(calls) % 3 == 2:
            buf[snap_off[index]:].view(np.int32)[where] = value
    sess = model._sess("_lp_batch_session", _lib_session())
    assert sess.deep_check is False
    with monkeypatch.context() as mp:
        mp.setattr(lpstate, "pack_snapshot", wrapper)
        got = model.score_lps(good, rank=True, return_exceptions=True)
        sel = model.select_cuts_lp_many(good, return_exceptions=True, **SELECT)
        with pytest.raises(ValueError, match=text):
            model.score_lps(good)
    assert len(calls) == 9
    for res in (got, sel):
        assert isinstance(res[1], ValueError) and text in str(res[1])
    # the neighbours' built states are those of a run without the bad snapshot; their scores are compared in a union of the same
    # shape, which the clean run is
    for at in (0, 2):
        assert _same_scores(got[at], clean[at]) and np.array_equal(got[at].rankings, clean[at].rankings)
        assert np.array_equal(sel[at].order, clean_sel[at].order) and sel[at].n_kept == clean_sel[at].n_kept
    after = model.score_lps(good, rank=True)
    assert all(_same_scores(a, b) for a, b in zip(after, clean))


def test_launch_record(model):
    names = ("rows1", "cuts257", "setcov-noinc")
    snaps, states = [_snap(n) for n in names], [_built_alone(model, n)[0] for n in names]
    model.score_lps(snaps), model.score_states(states)
    with _lib.launch_profile() as lp:
        model.score_lps(snaps)
    with _lib.launch_profile() as plain:
        model.score_states(states)
    got = [n for n, _ in lp.launches]
    assert got[:2] == ["k_lpset_stats", "k_lpset_emit"] and set(got[:2]) == NAMES
    assert got[2:] == [n for n, _ in plain.launches]


N_WORKERS = 4


def test_server_with_lp_workers(model, tmp_path):
    """Four torch-free workers that open no GPU send LP score, rank and select requests and one bad snapshot each."""
    address = str(tmp_path / "gcnn.sock")
    server = serve.ScoringServer({"m": model}, address)
    worker = os.path.join(ROOT, "tests", "serve_worker_lp.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, worker, ROOT, address, str(w), str(tmp_path / f"w{w}.npz"),
                               str(tmp_path / f"ready{w}")]) for w in range(N_WORKERS)]
    try:
        deadline = time.time() + 60
        while not all(os.path.exists(tmp_path / f"ready{w}") for w in range(N_WORKERS)):
            assert time.time() < deadline and all(p.poll() is None for p in procs), "a worker did not get ready"
            time.sleep(0.02)
        time.sleep(0.3)       # every worker's first request is waiting before the first sweep: it must group them
        server.start()
        codes = [p.wait(timeout=150) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        server.close()
    assert codes == [0] * N_WORKERS
    stats = server.stats
    assert stats["errors"] == N_WORKERS and stats["requests"] == N_WORKERS * (W.N_REQUESTS + 1)
    assert stats["batched_calls"] >= 1 and stats["max_batch"] >= 2, stats
    for w in range(N_WORKERS):
        got = np.load(tmp_path / f"w{w}.npz")
        for j in range(W.N_REQUESTS):
            kind, snap, forced = W.lp_request(w, j)
            q, index = got[f"s{j}"], got[f"i{j}"]
            assert q.dtype == np.float32 and index.dtype == np.int32
            if kind == "select":
                direct = model.select_cuts_lp(snap, forced, p_max=0.1, p_max_ub=0.5, max_selected=4)
                np.testing.assert_allclose(q, direct.scores.numpy(), rtol=1e-4, atol=1e-4)
                assert np.array_equal(index, direct.cut_index)
                state = model.state_from_lp(snap)[0]
                K, V = state[9], state[8]
                frows = None if forced is None else R.dense_rows(forced[0][0], forced[0][1], forced[1], forced[2], V)
                rec = {}
                order, n = R.select(q, R.dense_rows(state[5][0], state[5][1], state[6].reshape(-1), K, V), frows, 0.1, 0.5, record=rec)
                assert sorted(got[f"o{j}"].tolist()) == list(range(K))
                if R.margins_ok(rec, 0.1, 0.5):       # (a parallelism on a threshold is the restatement's to decline, not a failure)
                    assert np.array_equal(got[f"o{j}"], order) and int(got[f"n{j}"]) == n, (w, j)
            else:
                direct = model.score_lp(snap)
                np.testing.assert_allclose(q, direct.numpy(), rtol=1e-4, atol=1e-4)
                assert np.array_equal(index, direct.cut_index)
                if kind == "rank":
                    assert list(got[f"o{j}"]) == sorted(range(len(q)), key=lambda x: q[x], reverse=True), (w, j)
