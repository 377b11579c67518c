"""CPU checks of resident LPs behind the scoring server (serve.py: KIND_LP_OPEN / _ROUND / _CLOSE, `RemoteLPSession`): the wire
round trip of the three kinds; the requests of the kinds 0-6 still encode to the bytes they had before the new kinds came; and the
server's bookkeeping with stub models, sessions and a stub group, driven through `_read` and `_serve` without torch -- ownership by
connection, close on drop, the `max_sessions` error, a foreign id, two requests of one session in successive calls, 11 waiting
rounds as calls of 8 and 3, grouping by mode and thresholds."""
import hashlib
import struct
import types

import numpy as np
import pytest

from gcnn_cut_selector_amd import lpstate, serve
from servecommon import BLOCK, FORCED, Peer, StubModel, server_fixture, stub_server
from servecommon import open_session as _open, pump as _pump, same_fields as _same_fields, snap as _snap


def _state():
    f = lambda *s: (np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) / 8)    # noqa: E731
    cei = np.array([[0, 0, 1], [0, 2, 1]], np.int32)
    kei = np.array([[0, 1], [1, 2]], np.int32)
    return (f(2, 4), cei, f(3, 1), f(3, 14), f(2, 6), kei, f(2, 1), 2, 3, 2)


# (length, sha256) of the messages the encoders of the kinds 0-6 gave for the inputs above before the session kinds existed
BEFORE = {
    0: (521, "21b250555236ffecddc979d3a696c50de432d452120308a8decf12ca2e8cd742"),
    1: (521, "6382bba6afdc26da6bec00c95e1b88a9021ef64b50443bec63d5496fafe905ea"),
    2: (593, "ae249ae62a2859b97978981cab2e907a58c229912530675972f527b2112750b5"),
    3: (957, "c563a607782a8f7f855b86f07c123e5c59bc5f0505089f2c78785e742cc59b72"),
    4: (957, "fac778d389d840d964cb27ba861818827d03534a5b7234551bd8ab36e0cb7c5e"),
    5: (1029, "21e451d3db0e11f1855a36e428eed6a1362c99b14c8574d9728910d8c0c12e3c"),
    6: (472, "969db454ca849fa0f5be9bda3690792a20e4cfa201cb3a7a0932bc7f87d98bb4"),
}


def test_kinds_0_to_6_keep_their_bytes():
    msgs = {0: serve.encode_request("m", 0, _state()), 1: serve.encode_request("m", 1, _state()),
            2: serve.encode_request("m", 2, _state(), FORCED, 0.2, 0.6, 3), 3: serve.encode_lp_request("m", 3, _snap()),
            4: serve.encode_lp_request("m", 4, _snap()), 5: serve.encode_lp_request("m", 5, _snap(), FORCED, 0.2, 0.6, 3),
            6: serve.encode_hybrid_request("m", _snap(), FORCED, 0.2, 0.6, 3)}
    for kind, m in msgs.items():
        assert (len(m), hashlib.sha256(m).hexdigest()) == BEFORE[kind], kind
        assert serve.decode_request(m)["kind"] == kind
    assert (serve.KIND_SCORE, serve.KIND_RANK, serve.KIND_SELECT, serve.KIND_LP_SCORE, serve.KIND_LP_RANK, serve.KIND_LP_SELECT,
            serve.KIND_HYBRID_SELECT, serve.KIND_LP_OPEN, serve.KIND_LP_ROUND, serve.KIND_LP_CLOSE) == tuple(range(10))


ROUND_NAMES = [n for n, _ in lpstate.ROUND_FIELDS]


def test_wire_round_trip_of_the_session_kinds():
    snap = _snap()
    rows, rnd = lpstate.LPRows.from_snapshot(snap), lpstate.LPRound.from_snapshot(snap)
    req = serve.decode_request(serve.encode_open_request("setcov/0", rows, deep=False))
    assert (req["kind"], req["model_key"], req["deep"]) == (serve.KIND_LP_OPEN, "setcov/0", False)
    _same_fields(req["rows"], rows, [n for n, _ in lpstate.ROW_FIELDS])
    assert req["rows"].scalars() == rows.scalars()
    assert serve.decode_request(serve.encode_open_request("m", rows))["deep"] is True
    # a full round with a block and forced rows
    req = serve.decode_request(serve.encode_round_request("m", 41, serve.SESSION_SELECT, rnd, FORCED, 0.2, 0.6, 3, append=BLOCK))
    assert (req["kind"], req["session"], req["mode"], req["p_max"], req["p_max_ub"], req["max_selected"]) == (serve.KIND_LP_ROUND, 41, 2, 0.2, 0.6, 3)
    _same_fields(req["round"], rnd, ROUND_NAMES)
    assert req["round"].has_incumbent is rnd.has_incumbent and req["incremental"] is False
    _same_fields(req["block"], BLOCK, ("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs"))
    assert np.array_equal(req["forced"][0], FORCED[0]) and np.array_equal(req["forced"][1], FORCED[1]) and req["forced"][2] == 1
    # the presence mask: any subset of the optional arrays, has_incumbent None / False / True
    for drop, inc in ((("col_lb",), None), (("col_ub", "col_primal"), True), (lpstate.OPTIONAL, False), ((), None)):
        import dataclasses
        part = dataclasses.replace(rnd, **{n: None for n in drop}, has_incumbent=inc)
        for mode in (serve.SESSION_SCORE, serve.SESSION_RANK):
            req = serve.decode_request(serve.encode_round_request("m", 7, mode, part))
            assert req["mode"] == mode and req["block"] is None and req["forced"] is None and req["max_selected"] is None
            _same_fields(req["round"], part, ROUND_NAMES)
            assert req["round"].has_incumbent is inc
    # an append alone, and a close
    req = serve.decode_request(serve.encode_round_request("m", 9, serve.SESSION_APPEND, append=BLOCK, incremental=True))
    assert req["mode"] == serve.SESSION_APPEND and req["round"] is None and req["incremental"] is True and req["session"] == 9
    _same_fields(req["block"], BLOCK, ("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs"))
    req = serve.decode_request(serve.encode_close_request("m", 12))
    assert (req["kind"], req["session"]) == (serve.KIND_LP_CLOSE, 12)
    with pytest.raises(ValueError, match="block"):
        serve.encode_round_request("m", 9, serve.SESSION_APPEND)
    # malformed: a wrong array count for the header's word, an unknown mode, trailing bytes, an unknown kind
    good = bytearray(serve.encode_round_request("m", 7, serve.SESSION_SCORE, rnd))
    for spoil in (lambda b: b.__setitem__(5, b[5] + 1), lambda b: b.extend(b"\0"),
                  lambda b: struct.pack_into("<i", b, serve._REQ.size - 8, 4), lambda b: b.__setitem__(4, 10)):
        bad = bytearray(good)
        spoil(bad)
        with pytest.raises(serve.ProtocolError):
            serve.decode_request(bytes(bad))


# ---- the server's bookkeeping, with stubs ------------------------------------------------------------------------------------------------
class StubSession:
    def __init__(self, model, rows, deep):
        self.model, self.rows, self.deep, self.closed, self.appended = model, rows, deep, False, []

    def append_rows(self, *arrays, incremental=False):
        self.appended.append((arrays, incremental))

    def close(self):
        self.closed = True


class StubGroup:
    """Answers a member with its round's cut count; a round whose row_dual[0] is negative gets a ValueError in its slot.  Keeps
    `LPSessionGroup`'s counters: a selection or a scoring is one batched call, a ranking is left to the sessions' own calls."""

    def __init__(self):
        self.log, self.calls, self.max_sessions_per_call, self.solo_rounds = [], 0, 0, 0

    def _count(self, n, batched):
        if batched:
            self.calls, self.max_sessions_per_call = self.calls + 1, max(self.max_sessions_per_call, n)
        else:
            self.solo_rounds += n

    def _answers(self, rounds, make):
        return [ValueError("LP snapshot rejected by the device: stub") if r.row_dual[0] < 0 else make(int(np.asarray(r.cut_lhs).shape[0]))
                for r in rounds]

    def score(self, sessions, rounds, rank=False, appends=None, return_exceptions=False):
        self.log.append(("rank" if rank else "score", list(sessions), list(rounds), list(appends)))
        self._count(len(sessions), not rank)

        def make(k):
            q = np.arange(k, dtype=np.float32).view(serve.Scores)
            q.cut_index, q.rankings = np.arange(k, dtype=np.int32)[::-1], np.arange(k, dtype=np.int32)
            return q
        return self._answers(rounds, make)

    def select_cuts(self, sessions, rounds, forced=None, *, p_max, p_max_ub, max_selected=None, appends=None, return_exceptions=False):
        self.log.append(("select", list(sessions), list(rounds), list(appends), list(forced), p_max, p_max_ub))
        self._count(len(sessions), True)
        return self._answers(rounds, lambda k: types.SimpleNamespace(scores=np.arange(k, dtype=np.float32), order=np.arange(k, dtype=np.int32),
                                                                     cut_index=np.arange(k, dtype=np.int32)[::-1], n_kept=k))


server = server_fixture(lambda tmp_path: stub_server(tmp_path, {"a": StubModel("a", StubSession), "b": StubModel("b", StubSession)},
                                                     max_sessions=3, session_group=StubGroup()))


def _round(k=2, dual=0.25):
    snap = _snap()
    rnd = lpstate.LPRound.from_snapshot(snap)
    rnd.row_dual = np.array([dual, 0.0])
    if k != 2:
        rnd.cut_ptr, rnd.cut_col, rnd.cut_val = np.arange(k + 1, dtype=np.int32), np.zeros(k, np.int32), np.ones(k)
        rnd.cut_lhs, rnd.cut_rhs = np.full(k, -1e20), np.ones(k)
    return rnd


def test_ownership_close_on_drop_and_the_session_limit(server):
    p, q = Peer(server), Peer(server)
    s1, s2 = _open(server, p), _open(server, q, "b")
    assert s1 != s2 and server.stats["sessions_open"] == 2
    assert [len(m.opened) for m in server.models.values()] == [1, 1] and server.models["a"].opened[0].deep is True
    # a foreign id and an unknown id get an error reply; the server keeps serving
    q.send(serve.encode_round_request("b", s1, serve.SESSION_SCORE, _round()))
    p.send(serve.encode_close_request("a", 999))
    _pump(server, [p, q])
    for peer in (q, p):
        with pytest.raises(serve.ServerError, match="no LP session"):
            peer.reply()
    assert server._session_group.log == [] and server.stats["session_rounds"] == 0
    p.send(serve.encode_round_request("a", s1, serve.SESSION_RANK, _round(3)))
    _pump(server, [p, q])
    arrays, _, _ = p.reply()
    assert np.array_equal(arrays[0], [0, 1, 2]) and np.array_equal(arrays[1], [0, 1, 2]) and np.array_equal(arrays[2], [2, 1, 0])
    # the limit: a third session is the last one; an open beyond it gets an error reply
    s3 = _open(server, p)
    with pytest.raises(serve.ServerError, match="max_sessions"):
        _open(server, q)
    assert server.stats["sessions_open"] == 3
    # an append on its own reaches the session; a close frees the slot
    p.send(serve.encode_round_request("a", s3, serve.SESSION_APPEND, append=BLOCK, incremental=True))
    _pump(server, [p])
    assert p.reply()[0] == [] and server.models["a"].opened[1].appended[0][1] is True
    p.send(serve.encode_close_request("a", s3))
    _pump(server, [p])
    p.reply()
    assert server.models["a"].opened[1].closed and server.stats["sessions_open"] == 2
    assert _open(server, q) > s3
    # a connection that drops takes its sessions along, and only its own
    p.sock.close()
    _pump(server, [p, q])
    assert p.conn not in server._buffers and server.models["a"].opened[0].closed
    assert server.stats["sessions_open"] == 2 and not server.models["b"].opened[0].closed and not server.models["a"].opened[2].closed
    q.send(serve.encode_round_request("b", s1, serve.SESSION_SCORE, _round()))
    _pump(server, [q])
    with pytest.raises(serve.ServerError, match="no LP session"):
        q.reply()


def test_waiting_rounds_become_calls(server):
    server.max_sessions = 64
    group = server._session_group
    peers = [Peer(server) for _ in range(11)]
    ids = [_open(server, p, "ab"[i % 2]) for i, p in enumerate(peers)]
    sessions = {sid: server._sessions[sid][1] for sid in ids}
    # 11 waiting rounds of one mode and one pair of thresholds: calls of 8 and 3, across models, in arrival order
    for p, sid in zip(peers, ids):
        p.send(serve.encode_round_request("x", sid, serve.SESSION_SELECT, _round(), FORCED, 0.2, 0.6, 1, append=BLOCK))
    _pump(server, peers)
    assert [len(c[1]) for c in group.log] == [8, 3]
    assert [s for c in group.log for s in c[1]] == [sessions[sid] for sid in ids]
    assert all(c[0] == "select" and c[5:] == (0.2, 0.6) for c in group.log)
    assert all(a is not None and np.array_equal(a.row_col, BLOCK.row_col) for c in group.log for a in c[3])
    assert all(f[2] == 1 and np.array_equal(f[0], FORCED[0]) for c in group.log for f in c[4])
    for p in peers:
        arrays, n_kept, n_selected = p.reply()
        assert (n_kept, n_selected) == (2, 1) and np.array_equal(arrays[2], [1, 0])
    assert (server.stats["session_rounds"], server.stats["session_calls"], server.stats["max_sessions_per_call"]) == (11, 2, 8)
    # grouping by mode and thresholds: four groups, one call each; a member's device error stays in its slot
    del group.log[:]
    plan = [(serve.SESSION_SCORE, {}), (serve.SESSION_RANK, {}), (serve.SESSION_SELECT, dict(p_max=0.1, p_max_ub=0.5)),
            (serve.SESSION_SELECT, dict(p_max=0.1, p_max_ub=0.6)), (serve.SESSION_SCORE, {}), (serve.SESSION_SELECT, dict(p_max=0.1, p_max_ub=0.5))]
    for i, (p, sid, (mode, kw)) in enumerate(zip(peers, ids, plan)):
        p.send(serve.encode_round_request("x", sid, mode, _round(dual=-1.0 if i == 4 else 0.25), **kw))
    _pump(server, peers[:6])
    assert sorted((c[0], len(c[1])) + tuple(c[5:]) for c in group.log) == [("rank", 1), ("score", 2), ("select", 1, 0.1, 0.6), ("select", 2, 0.1, 0.5)]
    for i, p in enumerate(peers[:6]):
        if i == 4:
            with pytest.raises(ValueError, match="rejected by the device"):
                p.reply()
        else:
            p.reply()
    # the calls are the group's own count: the ranking it left to the session's own call is a solo round, not a call
    assert (server.stats["session_calls"], server.stats["session_solo_rounds"], server.stats["errors"]) == (5, 1, 1)
    assert server.stats["session_rounds"] == 17 and server.stats["max_sessions_per_call"] == 8
    # two requests of one session are never in one call: arrival order, successive calls
    del group.log[:]
    peers[0].send(serve.encode_round_request("x", ids[0], serve.SESSION_SCORE, _round(3)))
    peers[0].send(serve.encode_round_request("x", ids[0], serve.SESSION_SCORE, _round(5)))
    peers[1].send(serve.encode_round_request("x", ids[1], serve.SESSION_SCORE, _round(4)))
    _pump(server, peers[:2])
    assert [[np.asarray(r.cut_lhs).shape[0] for r in c[2]] for c in group.log] == [[3, 4], [5]]
    assert [s for s in group.log[1][1]] == [sessions[ids[0]]]
    assert [peers[0].reply()[0][0].shape[0], peers[0].reply()[0][0].shape[0], peers[1].reply()[0][0].shape[0]] == [3, 5, 4]


def test_remote_session_is_numpy_only():
    import subprocess
    import sys
    code = ("import sys; from gcnn_cut_selector_amd import serve; "
            "assert 'torch' not in sys.modules; s = serve.RemoteLPSession(None, 1, 5, 3); "
            "assert (s.n_rows, s.n_cols, s.closed) == (5, 3, False) and hasattr(serve.ScoringClient, 'open_lp'); "
            "assert all(hasattr(s, n) for n in ('score', 'select_cuts', 'append_rows', 'close', '__enter__', '__exit__'))")
    subprocess.run([sys.executable, "-c", code], check=True)
