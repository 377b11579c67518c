"""Host proofs for the data collector's expert round (collect.Collector.collect_lp, serve.KIND_COLLECT): the restatement of
tests/collectcases.py against its three planted defects, each caught by a named case; the cases' margins; every refusal the host
makes before anything is enqueued; improvements == quality[cut_index]; the wire round trip of kind 11, the bytes of the kinds 3-6
before and after, kind 10 still refused; the server's bookkeeping with a stub collector; the client's local refusals."""
import hashlib
import socket
import subprocess
import sys
import os

import numpy as np
import pytest

import collectcases as CC
import hybrid_restate as H
import hybridcases as X
from gcnn_cut_selector_amd import lpstate, serve
from servecommon import FORCED, Peer, server_fixture, stub_server
from servecommon import pump as _pump, snap as _snap
from test_lprounds_host import BEFORE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return np.array_equal(a["order"], b["order"]) and a["n_kept"] == b["n_kept"] and np.array_equal(a["improvements"], b["improvements"])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", CC.SIZES)
def test_snapshots_have_their_sizes_and_both_sides(K):
    ref = CC.state_ref(K)
    side, cut_index = ref["side_lhs"], ref["cut_index"]
    assert ref["dims"]["n_cuts"] == K and sorted(cut_index.tolist()) == list(range(K))
    assert (ref["margin"] > ref["margin_bound"]).all()              # no side choice sits at its tie
    if K > 1:
        assert side.any() and not side.all()
        assert side[np.flatnonzero(~side)[0]:].any()                 # an rhs-side cut in front of an lhs-side one:
        assert not np.array_equal(cut_index, np.arange(K))           # state order is not input order
    assert lpstate.check_snapshot(CC.too_many())[1]["n_cuts"] == 4097


@pytest.mark.parametrize("case", CC.GPU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_every_device_case_is_decided_far_from_a_parallelism_tie(case):
    K, name, n_forced, p_max, p_max_ub = case
    q, forced, record = CC.quality(K, name), CC.forced_rows(K, n_forced), {}
    ref = CC.restate(K, q, forced, p_max, p_max_ub, record=record)
    assert CC.parallelism_margin(record, p_max, p_max_ub) > CC.P_MARGIN
    assert sorted(ref["order"].tolist()) == list(range(K)) and 0 < ref["n_kept"] <= K
    assert np.array_equal(ref["improvements"], q[ref["cut_index"]])
    if K >= 63:
        assert ref["n_kept"] < K or name == "equal"                 # the filter removes cuts: a ranking alone would not pass
    # the float64 walk of tests/hybrid_restate.py, written independently, agrees
    order, n_kept = H.select(q, CC.rows_ref(K)["rows"], X.forced_dense(forced, CC.snapshot(K).col_type.shape[0]), p_max, p_max_ub)
    assert np.array_equal(order, ref["order"]) and n_kept == ref["n_kept"]


def test_quality_families_are_what_they_claim():
    for K in CC.SIZES[2:-1]:
        side = CC.state_ref(K)["side_lhs"]
        ties, neg, beyond = CC.quality(K, "ties"), CC.quality(K, "negative"), CC.quality(K, "beyond_fp32")
        # a tie between an rhs-side cut and a LATER lhs-side cut: input order and state order rank the pair differently
        assert any(side[j] and not side[i] and ties[i] == ties[j] for i in range(K) for j in range(i + 1, K))
        record = {}
        CC.restate(K, neg, record=record)
        assert neg.max() < 0 and 0.9 * neg.max() > neg.max() and record["low"].all()          # the first position included
        assert len(set(beyond.astype(np.float32).tolist())) == 2 and len(set(beyond.tolist())) == 3
        assert np.float32(0.9 * (1 - 2.0 ** -30)) == np.float32(0.9) == np.float32(0.9 * (1 + 2.0 ** -30))
        record32 = {}
        CC.restate(K, beyond, record=record)
        CC.restate(K, beyond, defect="fp32_threshold", record=record32)
        assert record["low"].sum() > 0 and record32["low"].sum() == 0                         # the float32 threshold flips flags
        assert len(set(CC.quality(K, "spread").tolist())) == K and len(set(CC.quality(K, "equal").tolist())) == 1


# ---- the planted defects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (63, 64, 65, 257, 4096))
def test_all_equal_qualities_catch_a_ranking_in_state_order(K):
    thr = (0.3, 0.6) if K == 4096 else (0.1, 0.5)
    q = CC.quality(K, "equal")
    good, bad = CC.restate(K, q, None, *thr), CC.restate(K, q, None, *thr, defect="state_order_ranking")
    assert not np.array_equal(good["order"], bad["order"])
    kept = good["order"][:good["n_kept"]]
    assert np.array_equal(kept, np.sort(kept))                       # the kept cuts stay in input order: the tie-break alone ranks


@pytest.mark.parametrize("K", (63, 64, 65, 257))
def test_each_defect_is_caught_by_its_named_case(K):
    caught = {"state_order_ranking": ("equal", "ties"), "fp32_threshold": ("beyond_fp32",),
              "input_order_improvements": ("ties", "negative", "beyond_fp32", "spread")}
    for defect, names in caught.items():
        for name in names:
            q = CC.quality(K, name)
            good, bad = CC.restate(K, q), CC.restate(K, q, defect=defect)
            assert not _same(good, bad), (defect, name)
            if defect == "fp32_threshold":
                assert (good["n_kept"], good["order"].tolist()) != (bad["n_kept"], bad["order"].tolist())
            if defect == "input_order_improvements":
                assert np.array_equal(good["order"], bad["order"]) and not np.array_equal(good["improvements"], bad["improvements"])
    # and a defect leaves alone what it does not touch: the restatement is not simply unstable
    q = CC.quality(K, "spread")
    assert _same(CC.restate(K, q), CC.restate(K, q, defect="state_order_ranking"))
    assert _same(CC.restate(K, q), CC.restate(K, q, defect="fp32_threshold"))


def test_with_the_hybrid_quality_the_restatement_is_the_hybrid_selection():
    """The issue's oracle, on the host: quality := the hybrid quality gives `hybrid_restate.select`'s order and n_kept."""
    for K in (65, 257):
        ref = CC.rows_ref(K)
        forced = CC.forced_rows(K, 3)
        want = H.select(ref["quality"], ref["rows"], X.forced_dense(forced, ref["dims"]["n_cols"]))
        got = CC.restate(K, ref["quality"], forced)
        assert np.array_equal(got["order"], want[0]) and got["n_kept"] == want[1]
        assert CC.restate(K, ref["quality"], forced, max_selected=5)["n_selected"] == min(5, want[1])


# ---- host refusals -----------------------------------------------------------------------------------------------------------------
def test_quality_refusals():
    q = lpstate.check_quality([0.5, 1, 0.25], 3)
    assert q.dtype == np.float64 and q.flags.c_contiguous and q.tolist() == [0.5, 1.0, 0.25]
    assert lpstate.check_quality(np.array([1, 2], np.int32), 2).dtype == np.float64
    assert lpstate.check_quality(np.zeros(0), 0).shape == (0,)
    for bad, text in ((np.zeros(2), "one value per cut"), (np.zeros((3, 1)), "one value per cut"), (np.zeros(4), "one value per cut"),
                      (np.array([0.0, np.nan, 1.0]), "finite"), (np.array([0.0, -np.inf, 1.0]), "finite"),
                      (np.array([0.0, np.inf, 1.0]), "finite"), (np.array(["a", "b", "c"]), "dtype"),
                      (np.array([True, False, True]), "dtype"), (np.array([1j, 0, 0]), "dtype")):
        with pytest.raises(ValueError, match=text):
            lpstate.check_quality(bad, 3)


def test_collect_lp_refuses_on_the_host_before_any_device_work():
    from gcnn_cut_selector_amd import _lib
    from gcnn_cut_selector_amd.collect import Collector
    col = Collector("cuda:0")                     # (no device is touched before the first call that passes the host's checks)
    snap = CC.snapshot(65)
    q = CC.quality(65, "spread")
    for bad in (q[:-1], np.where(np.arange(65) == 7, np.nan, q), np.where(np.arange(65) == 7, -np.inf, q), q.astype("U8")):
        with pytest.raises(ValueError):
            col.collect_lp(snap, bad)
    for thr in (dict(p_max=float("nan")), dict(p_max_ub=float("inf")), dict(p_max="0.1")):
        with pytest.raises(ValueError):
            col.collect_lp(snap, q, **thr)
    with pytest.raises(_lib.GcnnError, match="4097 cuts"):
        col.collect_lp(CC.too_many(), np.zeros(4097))
    with pytest.raises(ValueError):                                                  # forced rows over columns the LP does not have
        col.collect_lp(snap, q, (np.array([[0], [10 ** 6]], np.int32), np.ones(1, np.float32), 1))
    broken = lpstate.LPSnapshot(**{k: getattr(snap, k) for k in snap.__dataclass_fields__})
    broken.cut_ptr = broken.cut_ptr.copy()
    broken.cut_ptr[1] = broken.cut_ptr[0]
    with pytest.raises(ValueError, match="at least one entry"):
        col.collect_lp(broken, q)
    assert col._session is None                                                      # nothing was staged, nothing enqueued


# ---- the wire ----------------------------------------------------------------------------------------------------------------------
def _wire_same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_kind_11_round_trips_bit_for_bit():
    assert serve.KIND_COLLECT == 11
    snap = _snap()
    quality = np.array([0.25, -0.0])
    sent, dims = lpstate.check_snapshot(snap, deep=False)
    for forced, inc in ((None, True), (FORCED, True), (FORCED, False)):
        s = snap if inc else lpstate.LPSnapshot(**{**{k: getattr(snap, k) for k in snap.__dataclass_fields__},
                                                   "col_primal": None, "col_primal_avg": None})
        message = serve.encode_collect_request("whatever", s, quality, forced, 0.25, 0.75, 7)
        req = serve.decode_request(message)
        assert (req["kind"], req["p_max"], req["p_max_ub"], req["max_selected"]) == (11, 0.25, 0.75, 7)
        assert _wire_same(req["quality"], quality) and np.signbit(req["quality"][1])
        got, got_dims = lpstate.check_snapshot(req["snapshot"], deep=False)
        want, want_dims = lpstate.check_snapshot(s, deep=False)
        assert got_dims == want_dims and all(_wire_same(a, b) for a, b in zip(got, want))
        assert message[5] == (21 if inc else 19) + 2 + (2 if forced else 0)
        if forced is None:
            assert req["forced"] is None
        else:
            assert _wire_same(req["forced"][0], forced[0]) and _wire_same(req["forced"][1], forced[1]) and req["forced"][2] == 1
        head = message[:4]
        for bad in (message[:30], message[:-1], message + b"\0", head + bytes([10]) + message[5:], head + bytes([12]) + message[5:],
                    head + bytes([serve.KIND_LP_SELECT]) + message[5:], message[:5] + bytes([message[5] - 1]) + message[6:]):
            with pytest.raises(serve.ProtocolError):
                serve.decode_request(bad)
    # an LP selection relabelled as an expert round lacks the quality: the count check refuses it
    lp = serve.encode_lp_request("m", serve.KIND_LP_SELECT, snap, FORCED)
    with pytest.raises(serve.ProtocolError):
        serve.decode_request(lp[:4] + bytes([11]) + lp[5:])
    # a quality that is not a float64 vector is no request of this protocol
    message = serve.encode_collect_request("m", snap, quality)
    at = len(message) - 16 - serve._ARR.size
    assert serve._ARR.unpack_from(message, at)[:2] == (1, 1)
    bad = message[:at] + serve._ARR.pack(3, 1, 0, 2, 0, 16) + message[at + serve._ARR.size:]          # the same bytes as int64
    with pytest.raises(serve.ProtocolError, match="quality"):
        serve.decode_request(bad)


def test_kinds_3_to_6_keep_their_bytes_and_kind_10_stays_unknown():
    msgs = {3: serve.encode_lp_request("m", 3, _snap()), 4: serve.encode_lp_request("m", 4, _snap()),
            5: serve.encode_lp_request("m", 5, _snap(), FORCED, 0.2, 0.6, 3), 6: serve.encode_hybrid_request("m", _snap(), FORCED, 0.2, 0.6, 3)}
    for kind, m in msgs.items():
        assert (len(m), hashlib.sha256(m).hexdigest()) == BEFORE[kind], kind
        assert serve.decode_request(m)["kind"] == kind
    rnd = serve.encode_round_request("m", 1, serve.SESSION_SCORE, lpstate.LPRound.from_snapshot(_snap()))
    col = serve.encode_collect_request("m", _snap(), np.zeros(2))
    for m in (rnd, col, msgs[5]):
        with pytest.raises(serve.ProtocolError):
            serve.decode_request(m[:4] + bytes([10]) + m[5:])


def test_the_reply_carries_the_twelve_arrays():
    f = lambda *s: (np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) / 8)    # noqa: E731
    state = (f(2, 4), np.array([[0, 0, 1], [0, 2, 1]], np.int32), f(3, 1), f(3, 14), f(2, 6), np.array([[0, 1], [1, 2]], np.int32), f(2, 1))
    more = [np.array([1, 0], np.int32), np.array([0.5, 0.25]), np.array([1, 0], np.int32), np.array([0.1, np.nan]), np.zeros((2, 3))]
    arrays, n_kept, n_sel = serve.decode_reply(serve.encode_reply(list(state) + more, 2, 1))
    assert len(arrays) == 12 and (n_kept, n_sel) == (2, 1) and all(_wire_same(a, b) for a, b in zip(arrays, list(state) + more))
    empty = [np.zeros((0, 4), np.float32), np.zeros((2, 0), np.int32), np.zeros((0, 1), np.float32)]
    arrays, _, _ = serve.decode_reply(serve.encode_reply(empty))
    assert [a.shape for a in arrays] == [(0, 4), (2, 0), (0, 1)]


# ---- the server's bookkeeping, with a stub collector ------------------------------------------------------------------------------
class StubCollector:
    def __init__(self):
        self.log = []

    def collect_lp(self, snapshot, quality, forced=None, *, p_max, p_max_ub, max_selected=None):
        self.log.append((snapshot, quality, forced, p_max, p_max_ub, max_selected))
        if quality[0] < 0:
            raise ValueError("LP snapshot rejected by the device: stub")
        k = quality.shape[0]
        f = lambda *s: np.full(s, 0.5, np.float32)  # noqa: E731
        state = (f(3, 4), np.zeros((2, 4), np.int32), f(4, 1), f(3, 14), f(k, 6), np.zeros((2, 3), np.int32), f(3, 1), 3, 3, k)
        index = np.arange(k, dtype=np.int32)[::-1].copy()
        n_kept = k - 1
        return lpstate.CollectResult(state, index, quality[index], np.arange(k, dtype=np.int32), n_kept,
                                     n_kept if max_selected is None else min(n_kept, max_selected), quality + 1.0, np.ones((k, 3)))


server = server_fixture(lambda tmp_path: stub_server(tmp_path, {}, StubCollector()))           # no model at all


def test_server_answers_expert_rounds_one_by_one(server):
    assert server.stats["collect_calls"] == 0 and server._device() is None
    p, q = Peer(server), Peer(server)
    p.send(serve.encode_collect_request("no such model", _snap(), np.array([0.5, 0.25]), FORCED, 0.2, 0.6, 1))
    q.send(serve.encode_collect_request("another", _snap(), np.array([-1.0, 0.25])))      # the stub rejects it as the device would
    p.send(serve.encode_collect_request("", _snap(), np.array([0.0, 0.0])))
    _pump(server, [p, q])
    arrays, n_kept, n_sel = p.reply()
    assert len(arrays) == 12 and (n_kept, n_sel) == (1, 1)
    assert arrays[7].tolist() == [1, 0] and arrays[8].tolist() == [0.25, 0.5] and arrays[10].tolist() == [1.5, 1.25]
    assert arrays[0].shape == (3, 4) and arrays[1].shape == (2, 4) and arrays[11].shape == (2, 3)
    with pytest.raises(ValueError, match="stub"):
        q.reply()
    arrays, n_kept, n_sel = p.reply()                               # the second request of the first peer is served all the same
    assert (n_kept, n_sel) == (1, 1) and arrays[8].tolist() == [0.0, 0.0]
    log = server._collector.log
    assert len(log) == 3 and server.stats["collect_calls"] == 3 and server.stats["errors"] == 1 and server.stats["requests"] == 3
    assert server.stats["calls"] == 0                               # no grouped call was made: these are answered on their own
    assert (log[0][3], log[0][4], log[0][5]) == (0.2, 0.6, 1) and log[0][2][2] == 1 and log[1][2] is None and log[2][5] is None
    assert isinstance(log[0][0], lpstate.LPSnapshot) and log[0][1].dtype == np.float64
    # a request the protocol refuses gets its error and is not counted as a call
    m = serve.encode_collect_request("m", _snap(), np.zeros(2))
    q.send(m[:4] + bytes([10]) + m[5:])
    _pump(server, [q])
    with pytest.raises(ValueError):
        q.reply()
    assert server.stats["collect_calls"] == 3 and server.stats["errors"] == 2


# ---- the client --------------------------------------------------------------------------------------------------------------------
def test_client_refuses_locally_what_it_can_see(tmp_path):
    listener = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    listener.bind(str(tmp_path / "sock"))
    listener.listen(1)
    client = serve.ScoringClient(str(tmp_path / "sock"), "m", timeout=5)
    conn, _ = listener.accept()
    conn.setblocking(False)
    try:
        for bad in (np.zeros(3), np.array([0.0, np.nan]), np.array([np.inf, 0.0]), np.array(["a", "b"]), np.zeros((2, 1))):
            with pytest.raises(ValueError):
                client.collect_lp(_snap(), bad)
        with pytest.raises(BlockingIOError):
            conn.recv(1)                                            # nothing was sent
    finally:
        client.close(); conn.close(); listener.close()


def test_client_half_imports_neither_torch_nor_the_binding():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gcnn_cut_selector_amd.serve as s\n"
            "import gcnn_cut_selector_amd.lpstate as l\n"
            "assert s.ScoringClient.collect_lp and s.encode_collect_request and l.CollectResult and l.check_quality\n"
            "assert s.KIND_COLLECT == 11\n"
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.')]\n"
            "assert not bad, bad\n"
            "assert 'gcnn_cut_selector_amd._lib' not in sys.modules and 'gcnn_cut_selector_amd.collect' not in sys.modules\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
