"""CPU checks of removals behind the scoring server (serve.py: KIND_LP_ROUND with the header's last word set, `RemoteLPSession`'s
`remove=` and `remove_rows`): the wire round trip of rounds with a removal, with a block and a removal, and of the edit-alone
forms; requests without a removal against bytes assembled by hand from the documented header; the malformed cases; and the
server's bookkeeping with stub models, sessions and stub groups, driven through `_read` and `_serve` without torch."""
import types

import numpy as np
import pytest

from gcnn_cut_selector_amd import lpstate, serve
from servecommon import BLOCK, FORCED, Peer, StubModel, server_fixture, shut, stub_server
from servecommon import by_hand as _by_hand, open_session as _open, pump as _pump, same_fields as _same_fields, snap as _snap


ROUND_NAMES = [n for n, _ in lpstate.ROUND_FIELDS]
BLOCK_NAMES = ("row_ptr", "row_col", "row_val", "row_lhs", "row_rhs")


def test_wire_round_trip_with_removals():
    rnd = lpstate.LPRound.from_snapshot(_snap())
    # a round with a removal; the list keeps the order it was given in
    req = serve.decode_request(serve.encode_round_request("m", 5, serve.SESSION_RANK, rnd, remove=[3, 0, 2]))
    assert (req["kind"], req["session"], req["mode"]) == (serve.KIND_LP_ROUND, 5, serve.SESSION_RANK) and req["block"] is None
    assert req["remove"].dtype == np.int32 and np.array_equal(req["remove"], [3, 0, 2]) and req["forced"] is None
    _same_fields(req["round"], rnd, ROUND_NAMES)
    # a selection with a block, a removal and forced rows: the list lies behind the block and in front of the forced pair
    req = serve.decode_request(serve.encode_round_request("m", 41, serve.SESSION_SELECT, rnd, FORCED, 0.2, 0.6, 3, append=BLOCK,
                                                          remove=np.array([1, 4], np.int64)))
    assert (req["mode"], req["p_max"], req["p_max_ub"], req["max_selected"]) == (serve.SESSION_SELECT, 0.2, 0.6, 3)
    _same_fields(req["round"], rnd, ROUND_NAMES)
    _same_fields(req["block"], BLOCK, BLOCK_NAMES)
    assert np.array_equal(req["remove"], [1, 4]) and req["remove"].dtype == np.int32
    assert np.array_equal(req["forced"][0], FORCED[0]) and np.array_equal(req["forced"][1], FORCED[1]) and req["forced"][2] == 1
    # the edit-alone forms: a list, a block, both
    req = serve.decode_request(serve.encode_round_request("m", 9, serve.SESSION_APPEND, remove=[7]))
    assert req["mode"] == serve.SESSION_APPEND and req["round"] is None and req["block"] is None and np.array_equal(req["remove"], [7])
    req = serve.decode_request(serve.encode_round_request("m", 9, serve.SESSION_APPEND, append=BLOCK, incremental=True))
    assert req["remove"] is None and req["incremental"] is True
    _same_fields(req["block"], BLOCK, BLOCK_NAMES)
    req = serve.decode_request(serve.encode_round_request("m", 9, serve.SESSION_APPEND, append=BLOCK, remove=[0, 3]))
    _same_fields(req["block"], BLOCK, BLOCK_NAMES)
    assert np.array_equal(req["remove"], [0, 3]) and req["round"] is None
    with pytest.raises(ValueError, match="block to append or rows to remove"):
        serve.encode_round_request("m", 9, serve.SESSION_APPEND)
    # a request without a removal decodes with none
    assert serve.decode_request(serve.encode_round_request("m", 7, serve.SESSION_SCORE, rnd))["remove"] is None


def test_requests_without_a_removal_keep_their_bytes():
    """The old bytes, pinned independently of the encoder: the header's last word is 0 and no array is added."""
    rnd = lpstate.LPRound.from_snapshot(_snap())
    arrays = [np.asarray(getattr(rnd, n)).astype(dt) for n, dt in lpstate.ROUND_FIELDS]
    block = [BLOCK.row_ptr, BLOCK.row_col, BLOCK.row_val, BLOCK.row_lhs, BLOCK.row_rhs]
    inc = 0 if rnd.has_incumbent is None else 2 if rnd.has_incumbent else 1
    word = lambda mode, has_block=0, incremental=0: mode | 15 << 8 | has_block << 12 | inc << 13 | incremental << 15  # noqa: E731
    assert serve.encode_round_request("m", 7, serve.SESSION_SCORE, rnd) == _by_hand(8, b"m", arrays, 0.1, 0.5, a=7, b=word(0))
    assert serve.encode_round_request("m", 7, serve.SESSION_RANK, rnd, append=BLOCK) == _by_hand(8, b"m", arrays + block, 0.1, 0.5, a=7,
                                                                                                 b=word(1, 1))
    assert serve.encode_round_request("key", 41, serve.SESSION_SELECT, rnd, FORCED, 0.2, 0.6, 3, append=BLOCK) == _by_hand(
        8, b"key", arrays + block + [FORCED[0], FORCED[1]], 0.2, 0.6, 3, 1, 41, word(2, 1))
    assert serve.encode_round_request("m", 9, serve.SESSION_APPEND, append=BLOCK, incremental=True) == _by_hand(
        8, b"m", block, 0.1, 0.5, a=9, b=3 | 1 << 12 | 1 << 15)
    assert serve.encode_close_request("m", 12) == _by_hand(9, b"m", [], a=12)
    # and with a removal: the last word is 1, the list is one more int32 array at its place
    lst = np.array([3, 0], np.int32)
    assert serve.encode_round_request("key", 41, serve.SESSION_SELECT, rnd, FORCED, 0.2, 0.6, 3, append=BLOCK, remove=[3, 0]) == _by_hand(
        8, b"key", arrays + block + [lst, FORCED[0], FORCED[1]], 0.2, 0.6, 3, 1, 41, word(2, 1), 1)
    assert serve.encode_round_request("m", 9, serve.SESSION_APPEND, remove=[3, 0]) == _by_hand(8, b"m", [lst], 0.1, 0.5, a=9, b=3, c=1)
    assert (serve.KIND_LP_OPEN, serve.KIND_LP_ROUND, serve.KIND_LP_CLOSE) == (7, 8, 9)
    assert (serve.SESSION_SCORE, serve.SESSION_RANK, serve.SESSION_SELECT, serve.SESSION_APPEND) == (0, 1, 2, 3)


def test_malformed_removals():
    rnd = lpstate.LPRound.from_snapshot(_snap())
    arrays = [np.asarray(getattr(rnd, n)).astype(dt) for n, dt in lpstate.ROUND_FIELDS]
    word = 15 << 8 | (0 if rnd.has_incumbent is None else 2 if rnd.has_incumbent else 1) << 13
    lst = np.array([1], np.int32)
    assert serve.decode_request(_by_hand(8, b"m", arrays + [lst], a=7, b=word, c=1))["remove"].tolist() == [1]
    bad = [_by_hand(8, b"m", arrays, a=7, b=word, c=1),                                  # the flag set but the array absent
           _by_hand(8, b"m", arrays + [lst], a=7, b=word, c=0),                          # the array without the flag
           _by_hand(8, b"m", arrays + [lst.astype(np.int64)], a=7, b=word, c=1),         # a list of the wrong dtype
           _by_hand(8, b"m", arrays + [lst.astype(np.float64)], a=7, b=word, c=1),
           _by_hand(8, b"m", arrays + [lst.reshape(1, 1)], a=7, b=word, c=1),            # or rank
           _by_hand(8, b"m", arrays + [lst], a=7, b=word, c=2),                          # a last word that is neither 0 nor 1
           _by_hand(8, b"m", [], a=7, b=3, c=0),                                         # edit-alone with neither block nor list
           _by_hand(8, b"m", [lst], a=7, b=3 | 1 << 8, c=1),                             # edit-alone with a presence mask
           _by_hand(8, b"m", [lst], a=7, b=4, c=1),                                      # no new mode
           _by_hand(10, b"m", [lst], a=7, b=3, c=1)]                                     # and no new kind
    for m in bad:
        with pytest.raises(serve.ProtocolError):
            serve.decode_request(m)


# ---- the server's bookkeeping, with stubs ------------------------------------------------------------------------------------------------
class StubSession:
    def __init__(self, model, rows, deep):
        self.model, self.rows, self.deep, self.closed, self.edits = model, rows, deep, False, []
        self.n_rows = int(np.asarray(rows.row_lhs).shape[0])

    def append_rows(self, *arrays, incremental=False):
        self.edits.append(("append", arrays, incremental))
        self.n_rows += int(np.asarray(arrays[3]).shape[0])

    def remove_rows(self, idx):
        self.edits.append(("remove", np.asarray(idx).tolist()))
        self.n_rows -= len(idx)

    def close(self):
        self.closed = True


class OldStubGroup:
    """A group from before removals: its calls take no `removes`.  Answers a member with its round's cut count."""

    def __init__(self):
        self.log, self.calls, self.max_sessions_per_call, self.solo_rounds = [], 0, 0, 0

    def _serve(self, what, sessions, rounds, make, **more):
        self.log.append(dict(what=what, sessions=list(sessions), rounds=list(rounds), **more))
        self.calls, self.max_sessions_per_call = self.calls + 1, max(self.max_sessions_per_call, len(sessions))
        return [make(int(np.asarray(r.cut_lhs).shape[0])) for r in rounds]

    @staticmethod
    def _scores(k):
        q = np.arange(k, dtype=np.float32).view(serve.Scores)
        q.cut_index, q.rankings = np.arange(k, dtype=np.int32)[::-1], np.arange(k, dtype=np.int32)
        return q

    @staticmethod
    def _selection(k):
        return types.SimpleNamespace(scores=np.arange(k, dtype=np.float32), order=np.arange(k, dtype=np.int32),
                                     cut_index=np.arange(k, dtype=np.int32)[::-1], n_kept=k)

    def score(self, sessions, rounds, rank=False, appends=None, return_exceptions=False):
        return self._serve("score", sessions, rounds, self._scores, appends=list(appends))

    def select_cuts(self, sessions, rounds, forced=None, *, p_max, p_max_ub, max_selected=None, appends=None, return_exceptions=False):
        return self._serve("select", sessions, rounds, self._selection, appends=list(appends))


class StubGroup(OldStubGroup):
    """Today's group: `removes` is a keyword of both calls; the log says whether a call got it."""

    def score(self, sessions, rounds, rank=False, appends=None, return_exceptions=False, **more):
        return self._serve("score", sessions, rounds, self._scores, appends=list(appends), **more)

    def select_cuts(self, sessions, rounds, forced=None, *, p_max, p_max_ub, max_selected=None, appends=None, return_exceptions=False, **more):
        return self._serve("select", sessions, rounds, self._selection, appends=list(appends), **more)


def _server(tmp_path, group):
    return stub_server(tmp_path, {"a": StubModel("a", StubSession), "b": StubModel("b", StubSession)}, session_group=group)


server = server_fixture(lambda tmp_path: _server(tmp_path, StubGroup()))


def _round(k=2):
    rnd = lpstate.LPRound.from_snapshot(_snap())
    if k != 2:
        rnd.cut_ptr, rnd.cut_col, rnd.cut_val = np.arange(k + 1, dtype=np.int32), np.zeros(k, np.int32), np.ones(k)
        rnd.cut_lhs, rnd.cut_rhs = np.full(k, -1e20), np.ones(k)
    return rnd


def test_rounds_with_and_without_removals_share_one_call(server):
    group = server._session_group
    peers = [Peer(server) for _ in range(4)]
    ids = [_open(server, p, "ab"[i % 2]) for i, p in enumerate(peers)]
    sessions = [server._sessions[sid][1] for sid in ids]
    removes = [None, [1], None, [0, 2]]
    appends = [None, None, BLOCK, BLOCK]
    for p, sid, a, r in zip(peers, ids, appends, removes):
        p.send(serve.encode_round_request("x", sid, serve.SESSION_SELECT, _round(), FORCED, 0.2, 0.6, 1, append=a, remove=r))
    _pump(server, peers)
    (call,) = group.log                                       # one mode, one pair of thresholds: one group call for all four
    assert call["what"] == "select" and call["sessions"] == sessions
    assert [None if r is None else r.tolist() for r in call["removes"]] == removes
    assert [a is not None for a in call["appends"]] == [False, False, True, True]
    for p in peers:
        arrays, n_kept, n_selected = p.reply()
        assert (n_kept, n_selected) == (2, 1)
    # a call in which no member removes: the keyword is not passed at all
    del group.log[:]
    for p, sid in zip(peers[:2], ids):
        p.send(serve.encode_round_request("x", sid, serve.SESSION_SCORE, _round(3)))
    _pump(server, peers[:2])
    (call,) = group.log
    assert call["what"] == "score" and "removes" not in call and len(call["sessions"]) == 2
    for p in peers[:2]:
        assert p.reply()[0][0].shape == (3,)
    assert (server.stats["session_rounds"], server.stats["session_calls"], server.stats["max_sessions_per_call"]) == (6, 2, 4)


def test_a_group_without_the_keyword_serves_removal_free_traffic(tmp_path):
    server = _server(tmp_path, OldStubGroup())
    try:
        peers = [Peer(server) for _ in range(2)]
        ids = [_open(server, p) for p in peers]
        for p, sid in zip(peers, ids):
            p.send(serve.encode_round_request("a", sid, serve.SESSION_SELECT, _round(), append=BLOCK))
        _pump(server, peers)
        assert len(server._session_group.log) == 1 and all(p.reply()[1] == 2 for p in peers)
        for p, sid in zip(peers, ids):
            p.send(serve.encode_round_request("a", sid, serve.SESSION_RANK, _round(3)))
        _pump(server, peers)
        assert all(p.reply()[0][1].shape == (3,) for p in peers) and server.stats["errors"] == 0
        # a removal it cannot take is that request's error; the server keeps serving
        peers[0].send(serve.encode_round_request("a", ids[0], serve.SESSION_SCORE, _round(), remove=[0]))
        peers[1].send(serve.encode_round_request("a", ids[1], serve.SESSION_RANK, _round()))
        _pump(server, peers)
        with pytest.raises(serve.ServerError, match="removes"):
            peers[0].reply()
        assert peers[1].reply()[0][0].shape == (2,)
    finally:
        shut(server)


def test_edits_alone_reach_the_session_and_the_client_counts_rows(server):
    peer = Peer(server)
    remote = serve.RemoteLPSession(peer, _open(server, peer), 2, 3)
    sess = server.models["a"].opened[0]
    remote.remove_rows([1])
    assert sess.edits == [("remove", [1])] and remote.n_rows == sess.n_rows == 1 and server._session_group.log == []
    remote.append_rows(*BLOCK.arrays(), incremental=True)
    assert sess.edits[-1][0] == "append" and sess.edits[-1][2] is True and remote.n_rows == sess.n_rows == 3
    remote.remove_rows([])                                    # nothing to remove: nothing is sent
    remote.remove_rows(None)
    assert len(sess.edits) == 2 and server.stats["requests"] == 3
    # both in one edit-alone request: the block without the row the list names in it, then the resident rows of the list
    peer.send(serve.encode_round_request("a", remote.session, serve.SESSION_APPEND, append=BLOCK, remove=[4, 0]))
    _pump(server, [peer])
    peer.reply()
    assert sess.edits[-2][0] == "append" and np.array_equal(sess.edits[-2][1][0], [0, 1]) and sess.edits[-1] == ("remove", [0])
    assert sess.n_rows == 3
    # rounds: n_rows follows the accepted edits, indices are numbered after the append
    remote._n_rows = 3
    sel = remote.select_cuts(_round(), FORCED, max_selected=1, append=BLOCK, remove=[4, 0, 2])
    assert remote.n_rows == 3 + 2 - 3 and (sel.n_kept, sel.n_selected) == (2, 1)
    call = server._session_group.log[-1]
    assert call["removes"][0].tolist() == [0, 2, 4] and call["appends"][0] is not None
    q = remote.score(_round(3), rank=True, remove=[1])
    assert remote.n_rows == 1 and q.shape == (3,) and np.array_equal(q.rankings, [0, 1, 2])
    # what the worker can see is refused in the worker, and counts nothing
    before = server.stats["requests"]
    for bad, match in (([1], r"outside \[0, 1\)"), ([0, 0], "twice"), ([0.5], "integers"), ([0], "no row at all")):
        with pytest.raises(ValueError, match=match):
            remote.score(_round(), remove=bad)
    with pytest.raises(ValueError, match="no row at all"):
        remote.remove_rows([0])
    assert remote.n_rows == 1 and server.stats["requests"] == before
    # an error of the server leaves the count alone
    foreign = serve.RemoteLPSession(peer, 999, 5, 3)
    with pytest.raises(serve.ServerError, match="no LP session"):
        foreign.remove_rows([2])
    assert foreign.n_rows == 5


def test_remote_session_with_removals_is_numpy_only():
    import subprocess
    import sys
    code = ("import sys, inspect; from gcnn_cut_selector_amd import serve; "
            "assert 'torch' not in sys.modules; s = serve.RemoteLPSession(None, 1, 5, 3); "
            "assert hasattr(s, 'remove_rows') and 'remove' in inspect.signature(s.score).parameters "
            "and 'remove' in inspect.signature(s.select_cuts).parameters")
    subprocess.run([sys.executable, "-c", code], check=True)
