"""CPU checks of the ensemble calls (gcnn_ensemble_mean, gcnn_infer_ensemble, gcnn_lp_ensemble) and of the server that uses them:
declared, exported and bound at ABI 13; launch names of their own file only; one kernel that cross-compiles for gfx950 as wave64
without LDS, scratch or atomics; limits and bad arguments returned without a device; a layout that uploads what gcnn_infer_batch
uploads for the one state; a server that answers an ensemble's name with the ensemble call and leaves the wire format alone."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

import buildsupport
import launchnames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcnn-cut-selector_amd", "csrc")
ENSEMBLE = os.path.join(CSRC, "gcnn_ensemble.hpp")
SYMBOLS = ("gcnn_ensemble_mean", "gcnn_infer_ensemble_layout_for", "gcnn_infer_ensemble", "gcnn_lp_ensemble_layout_for",
           "gcnn_lp_ensemble")
NAMES = {"k_ens_mean", "k_ens_unpack", "k_ens_by_variable", "k_ens_rank", "k_ens_lp_stats", "k_ens_lp_emit"}
ONE = (5, 6, 3, 7, 4)


def test_symbols_in_header_binding_and_library_abi_13():
    header = buildsupport.declared_everywhere(SYMBOLS)
    from gcnn_cut_selector_amd import _lib
    assert _lib.ABI_VERSION == 13 == _lib.lib().gcnn_abi_version()
    assert "gcnn_ensemble_layout" in header and "gcnn_lp_ensemble_layout" in header
    # every new entry cites the plugin that reads the result and the trainer that makes the five seeds
    for sym in ("gcnn_ensemble_mean is", "gcnn_infer_ensemble (", "gcnn_lp_ensemble ("):
        at = header.index(sym)
        text = header[at:at + 400]
        assert "model_evaluator.py:82-154" in text and "model_trainer.py:38-49" in text, sym


def test_launch_names_are_its_own():
    names = launchnames.launch_names(ENSEMBLE)
    assert names == NAMES
    assert not names & launchnames.launch_names()
    for other in sorted(os.listdir(CSRC)):
        if other.startswith("gcnn_") and other.endswith(".hpp") and other != "gcnn_ensemble.hpp":
            assert not names & launchnames.launch_names(os.path.join(CSRC, other)), other
    buildsupport.included_once_after("gcnn_ensemble.hpp", "gcnn_select.hpp", "gcnn_group.hpp", "gcnn_ibatch.hpp", "gcnn_lpbatch.hpp")
    # the forward passes go out under the group kernels' names: this file spells none of them
    assert "k_group_" not in re.sub(r"//[^\n]*", "", open(ENSEMBLE).read())


def test_kernel_compiles_wave64_without_lds_scratch_or_atomics():
    build = buildsupport.device_build()
    new = {k: v for k, v in build.rows.items() if "k_ens_" in k}
    assert len(new) == 1 and "k_ens_mean" in next(iter(new)), sorted(new)
    for name, v in new.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (name, v)
        assert not re.search(r"atomic", build.body(name)), name
        assert build.wavefront_size(name) == 64, name
    # the families the other build tests count are as they were
    rows = list(build.rows)
    assert sum("k_ib_" in r for r in rows) == 2 and sum("k_sel_" in r for r in rows) == 2 and sum("k_group_" in r for r in rows) == 35


def _layout(shape=ONE, forced=(0, 0), mode=0, M=3):
    from gcnn_cut_selector_amd import _lib
    L = _lib.EnsembleLayout()
    d = _lib.Dims(*shape)
    return _lib.lib().gcnn_infer_ensemble_layout_for(C.byref(d), forced[0], forced[1], mode, M, C.byref(L)), L, d


def _lp_dims(n_cuts=3, n_cols=6):
    from gcnn_cut_selector_amd import _lib
    return _lib.LpDims(n_rows=4, n_cols=n_cols, n_cuts=n_cuts, row_nnz=8, cut_nnz=2 * n_cuts, has_incumbent=0, n_model_vars=n_cols,
                       n_state_rows=4, n_state_edges=8, reserved=0, infinity=1e20, sum_epsilon=1e-6, obj_norm=1.0)


def _lp_layout(d, forced=(0, 0), mode=0, M=3):
    from gcnn_cut_selector_amd import _lib
    L = _lib.LpEnsembleLayout()
    return _lib.lib().gcnn_lp_ensemble_layout_for(C.byref(d), forced[0], forced[1], mode, M, C.byref(L)), L


def test_layout_refusals_without_a_device():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    assert _layout()[0] == 0 and _layout(M=1)[0] == 0 and _layout(M=8)[0] == 0
    assert _layout(M=0)[0] == -1 and _layout(M=9)[0] == -1
    assert _layout(mode=3)[0] == -1 and _layout(mode=-1)[0] == -1 and _layout(shape=(5, 6, -1, 7, 4))[0] == -1
    assert _layout(forced=(-1, 0), mode=2)[0] == -1 and _layout(forced=(0, 3), mode=2)[0] == -1
    d = _lib.Dims(*ONE)
    assert lib.gcnn_infer_ensemble_layout_for(C.byref(d), 0, 0, 0, 3, None) == -1
    assert lib.gcnn_infer_ensemble_layout_for(None, 0, 0, 0, 3, C.byref(_lib.EnsembleLayout())) == -1
    # 4,097 cuts: the two ordering modes decline, score mode answers; 4,096 are fine everywhere
    big = (5, 6, 4097, 7, 4097)
    assert _layout(big, mode=0)[0] == 0 and _layout(big, mode=1)[0] == -4 and _layout(big, mode=2)[0] == -4
    assert all(_layout((5, 6, 4096, 7, 4096), mode=m)[0] == 0 for m in (0, 1, 2))
    # more than 32,768 variables; edges with nothing to point at
    assert _layout((5, 32769, 3, 7, 4))[0] == -4 and _layout((5, 32768, 3, 7, 4))[0] == 0
    assert _layout((0, 5, 5, 3, 5))[0] == -4
    # the LP form: the same for the built state's sizes
    assert _lp_layout(_lp_dims())[0] == 0
    assert _lp_layout(_lp_dims(), M=0)[0] == -1 and _lp_layout(_lp_dims(), M=9)[0] == -1
    assert _lp_layout(_lp_dims(n_cuts=4097), mode=0)[0] == 0
    assert _lp_layout(_lp_dims(n_cuts=4097), mode=1)[0] == -4 and _lp_layout(_lp_dims(n_cuts=4097), mode=2)[0] == -4
    assert _lp_layout(_lp_dims(n_cols=32769))[0] == -4
    assert lib.gcnn_lp_ensemble_layout_for(C.byref(_lp_dims()), 0, 0, 0, 3, None) == -1


def test_layout_uploads_one_state_and_holds_every_member():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    shape, forced = (500, 1000, 100, 25000, 9000), (40, 800)
    dims = (_lib.Dims * 1)(_lib.Dims(*shape))
    for mode in (0, 1, 2):
        nf, nfe = (C.c_int32 * 1)(forced[0]), (C.c_int32 * 1)(forced[1])
        IL = _lib.IbatchLayout()
        assert lib.gcnn_infer_batch_layout_for(1, dims, nf, nfe, mode, C.byref(IL)) == 0
        ws = 4 * lib.gcnn_workspace_floats(C.byref(dims[0]))
        size = C.c_size_t()
        for M in (1, 5, 8):
            rc, EL, _ = _layout(shape, forced, mode, M)
            assert rc == 0 and EL.n_models == M
            L = EL.u
            # the upload is gcnn_infer_batch's for this one state, whatever M is
            assert L.in_bytes == IL.in_bytes and list(L.in_off) == list(IL.in_off) and list(L.out_off) == list(IL.out_off)
            dev_off = list(L.dev_off)
            assert all(o % 256 == 0 for o in dev_off + [EL.table_off, L.arena_bytes]) and dev_off[:14] == sorted(dev_off[:14])
            # the download reaches over the members' rows, which lie behind the output block and in front of the workspaces
            assert EL.member_stride >= 4 * shape[2] and EL.member_stride % 16 == 0
            assert EL.member_off >= IL.out_bytes and L.out_bytes == EL.member_off + M * EL.member_stride
            end = dev_off[11] + L.out_bytes
            for m in range(M):
                assert EL.ws_off[m] % 256 == 0 and EL.ws_off[m] >= end
                end = EL.ws_off[m] + ws
            assert end <= dev_off[13]
            assert lib.gcnn_group_table_bytes(M, C.byref(size)) == 0 and EL.table_bytes == size.value
            assert EL.table_off >= dev_off[13] and EL.table_off + EL.table_bytes <= L.arena_bytes


def test_ensemble_mean_bad_arguments_launch_nothing():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    fake = 1 << 20
    rows = (C.c_void_p * 8)(*([fake] * 8))
    assert lib.gcnn_ensemble_mean(rows, 0, 4, fake, None) == -1 and lib.gcnn_ensemble_mean(rows, 9, 4, fake, None) == -1
    assert lib.gcnn_ensemble_mean(rows, 3, -1, fake, None) == -1
    assert lib.gcnn_ensemble_mean(None, 3, 4, fake, None) == -1 and lib.gcnn_ensemble_mean(rows, 3, 4, None, None) == -1
    assert lib.gcnn_ensemble_mean((C.c_void_p * 3)(fake, None, fake), 3, 4, fake, None) == -1
    # n == 0 launches nothing, whatever the pointers are
    assert lib.gcnn_ensemble_mean(None, 3, 0, None, None) == 0 and lib.gcnn_ensemble_mean(rows, 8, 0, fake, None) == 0


def test_calls_refuse_bad_arguments_before_anything_is_enqueued():
    from gcnn_cut_selector_amd import _lib
    lib = _lib.lib()
    rc, EL, d = _layout(mode=2)
    assert rc == 0
    fake = 1 << 20
    params = (C.c_void_p * 3)(fake, fake + 4096, fake + 8192)

    def call(p_max=0.1, arena=fake * 256, size=EL.u.arena_bytes, par=params, host_in=fake, host_out=fake, staging=fake, M=3, mode=2):
        return lib.gcnn_infer_ensemble(C.byref(d), 0, 0, mode, M, par, host_in, host_out, arena, size, staging, p_max, 0.5, None)

    assert call(p_max=float("nan")) == -1 and call(p_max=float("inf")) == -1
    assert call(size=EL.u.arena_bytes - 1) == -1 and call(arena=fake * 256 + 16) == -1
    assert call(par=None) == -1 and call(par=(C.c_void_p * 3)(fake, None, fake)) == -1
    assert call(host_in=None) == -1 and call(host_out=None) == -1 and call(staging=None) == -1
    assert call(M=0) == -1 and call(M=9) == -1 and call(mode=3) == -1
    ld = _lp_dims()
    rc, L = _lp_layout(ld, mode=2)
    assert rc == 0

    def lp_call(p_max=0.1, size=L.lp.arena_bytes, par=params, host_in=fake, staging=fake, M=3):
        return lib.gcnn_lp_ensemble(C.byref(ld), 0, 0, 2, M, par, host_in, fake, fake * 256, size, staging, p_max, 0.5, None)

    assert lp_call(p_max=float("nan")) == -1 and lp_call(size=L.lp.arena_bytes - 1) == -1 and lp_call(par=None) == -1
    assert lp_call(host_in=None) == -1 and lp_call(staging=None) == -1 and lp_call(M=9) == -1


# ---- the server's bookkeeping, with stub models ----------------------------------------------------------------------------------------
class _Result(np.ndarray):
    rankings = None
    cut_index = None
    members = None


def _scores(tag):
    res = np.full(2, float(tag), np.float32).view(_Result)
    res.rankings, res.cut_index, res.members = np.array([1, 0], np.int32), np.array([0, 1], np.int32), np.zeros((2, 2), np.float32)
    return res


class _Selection:
    def __init__(self, tag):
        self.scores, self.order, self.n_kept, self.cut_index = _scores(tag), np.array([1, 0], np.int32), 1, np.array([0, 1], np.int32)
        self.members = np.zeros((2, 2), np.float32)


class _StubModel:
    device = "stub"

    def __init__(self, log, name):
        self.log, self.name = log, name

    def score_states(self, states, rank=False, return_exceptions=False):
        self.log.append(("model", self.name, "score_states", len(states)))
        return [_scores(1) for _ in states]

    def select_cuts_many(self, states, forced=None, **kw):
        self.log.append(("model", self.name, "select_cuts_many", len(states)))
        return [_Selection(1) for _ in states]

    def score_lps(self, snaps, rank=False, return_exceptions=False):
        self.log.append(("model", self.name, "score_lps", len(snaps)))
        return [_scores(1) for _ in snaps]

    def select_cuts_lp_many(self, snaps, forced=None, **kw):
        self.log.append(("model", self.name, "select_cuts_lp_many", len(snaps)))
        return [_Selection(1) for _ in snaps]


class _StubSet:
    def __init__(self, log):
        self.log = log

    def score_ensemble(self, keys, state, rank=False):
        self.log.append(("ensemble", "score_ensemble", tuple(keys), bool(rank)))
        return _scores(7)

    def select_cuts_ensemble(self, keys, state, forced=None, *, p_max, p_max_ub, max_selected):
        self.log.append(("ensemble", "select_cuts_ensemble", tuple(keys), (p_max, p_max_ub, max_selected)))
        return _Selection(7)

    def score_lp_ensemble(self, keys, snap, rank=False):
        self.log.append(("ensemble", "score_lp_ensemble", tuple(keys), bool(rank)))
        return _scores(7)

    def select_cuts_lp_ensemble(self, keys, snap, forced=None, *, p_max, p_max_ub, max_selected):
        self.log.append(("ensemble", "select_cuts_lp_ensemble", tuple(keys), (p_max, p_max_ub, max_selected)))
        return _Selection(7)


class _FakeConn:
    """A connection the server can read requests from and write replies to, without a socket."""

    def __init__(self):
        self.inbox, self.sent = [], []

    def recv(self, n):
        return self.inbox.pop(0)

    def sendall(self, data):
        self.sent.append(bytes(data))

    def close(self):
        pass


def _frame(message):
    import struct
    return struct.pack("<I", len(message)) + message


def _server(tmp, log, **kw):
    from gcnn_cut_selector_amd import serve
    return serve.ScoringServer({k: _StubModel(log, k) for k in "abc"}, os.path.join(tmp, "s.sock"), model_set=_StubSet(log), **kw)


def _requests():
    """One request of every kind 0-5 (as (kind, message under `key`)) and the state and snapshot they carry."""
    from gcnn_cut_selector_amd import serve, synthetic, utils
    state = utils.state_to_inputs(synthetic.make_sample("setcov", 1, scale=0.2)[0])
    snap = synthetic.make_lp_snapshot("setcov", 1, scale=0.2, n_cuts=3)

    def make(key):
        out = [(k, serve.encode_request(key, k, state, p_max=0.2, p_max_ub=0.6, max_selected=4))
               for k in (serve.KIND_SCORE, serve.KIND_RANK, serve.KIND_SELECT)]
        return out + [(k, serve.encode_lp_request(key, k, snap, p_max=0.2, p_max_ub=0.6, max_selected=4))
                      for k in (serve.KIND_LP_SCORE, serve.KIND_LP_RANK, serve.KIND_LP_SELECT)]
    return make, state, snap


def test_server_refuses_bad_ensembles():
    from gcnn_cut_selector_amd import serve
    with tempfile.TemporaryDirectory() as tmp:
        for bad in ({"a": ["b", "c"]}, {"ens": ["a", "nobody"]}, {"ens": []}, {"ens": ["a", "a"]}, {"ens": list("abcabcabc")}):
            with pytest.raises(ValueError):
                _server(tmp, [], ensembles=bad)
            assert not os.path.exists(os.path.join(tmp, "s.sock")), "a refused server leaves no socket behind"
        with pytest.raises(ValueError):                  # models on two devices cannot share the ensemble's ModelSet
            models = {k: _StubModel([], k) for k in "ab"}
            models["b"].device = "elsewhere"
            serve.ScoringServer(models, os.path.join(tmp, "s.sock"), ensembles={"ens": ["a", "b"]})
        server = _server(tmp, [], ensembles={"ens": ["c", "a"]})
        try:
            assert server.ensembles == {"ens": ["c", "a"]} and server.stats["ensemble_calls"] == 0
        finally:
            server.close()
    assert serve.ScoringServer.__init__.__defaults__[1] is True


def test_an_ensemble_name_reaches_the_ensemble_call_and_the_wire_bytes_are_what_they_were():
    from gcnn_cut_selector_amd import serve
    make, state, snap = _requests()
    log = []
    with tempfile.TemporaryDirectory() as tmp:
        server = _server(tmp, log, ensembles={"ens": ["c", "a"]})
        try:
            # the request's bytes do not know whether the key names a model or an ensemble
            for (kind, under_ens), (_, under_abc) in zip(make("ens"), make("abc")):
                assert under_ens.replace(b"ens", b"abc") == under_abc and len(under_ens) == len(under_abc), kind
            conn, plain = _FakeConn(), _FakeConn()
            server._buffers[conn], server._buffers[plain] = bytearray(), bytearray()
            pending = []
            for (kind, message), (_, message_b) in zip(make("ens"), make("b")):
                conn.inbox.append(_frame(message))
                server._read(conn, pending)
                plain.inbox.append(_frame(message_b))
                server._read(plain, pending)
            assert len(pending) == 12 and not conn.sent and not plain.sent
            server._serve(pending)
        finally:
            server.close()
    # every ensemble request took its own ensemble call, in arrival order, with the ensemble's keys in their order
    mine = [e for e in log if e[0] == "ensemble"]
    assert mine == [("ensemble", "score_ensemble", ("c", "a"), False), ("ensemble", "score_ensemble", ("c", "a"), True),
                    ("ensemble", "select_cuts_ensemble", ("c", "a"), (0.2, 0.6, 4)),
                    ("ensemble", "score_lp_ensemble", ("c", "a"), False), ("ensemble", "score_lp_ensemble", ("c", "a"), True),
                    ("ensemble", "select_cuts_lp_ensemble", ("c", "a"), (0.2, 0.6, 4))]
    # the plain requests were served as before: one call per kind on model b, none of them shared with an ensemble request
    assert sorted(e[2] for e in log if e[0] == "model") == sorted(["score_states"] * 2 + ["select_cuts_many"] + ["score_lps"] * 2 +
                                                                  ["select_cuts_lp_many"])
    assert all(e[1] == "b" and e[3] == 1 for e in log if e[0] == "model")
    assert server.stats["ensemble_calls"] == 6 and server.stats["calls"] == 12 and server.stats["errors"] == 0
    # the replies: the existing shapes, the mean and not the members -- byte for byte what a model's result of those values gives
    assert len(conn.sent) == 6 and len(plain.sent) == 6
    kinds = [k for k, _ in make("ens")]
    for kind, sent in zip(kinds, conn.sent):
        lp, base = kind in serve._LP_BASE, serve._LP_BASE.get(kind, kind)
        if base == serve.KIND_SELECT:
            want = serve.encode_reply(*serve._selection_reply(_Selection(7), 4, lp))
            got = serve._selection_of(serve.decode_reply(sent[4:]), lp)
            assert got.scores.tolist() == [7.0, 7.0] and got.order.tolist() == [1, 0] and (got.n_kept, got.n_selected) == (1, 1)
        else:
            want = serve.encode_reply(*serve._scores_reply(_scores(7), base == serve.KIND_RANK, lp))
            got = serve._scores_of(serve.decode_reply(sent[4:]), base == serve.KIND_RANK, lp)
            assert got.tolist() == [7.0, 7.0] and (got.cut_index is not None) == lp
        assert sent == _frame(want), kind
        assert len(serve.decode_reply(sent[4:])[0]) == len(serve.decode_reply(plain.sent[kinds.index(kind)][4:])[0])


def test_other_kinds_under_an_ensemble_name_get_the_unknown_model_reply():
    import lpsessioncases
    from gcnn_cut_selector_amd import serve
    _, state, snap = _requests()
    rows, rnd = lpsessioncases.split(snap)
    quality = np.linspace(0.0, 1.0, 3)

    def others(key):
        return [(serve.KIND_HYBRID_SELECT, serve.encode_hybrid_request(key, snap)),
                (serve.KIND_LP_OPEN, serve.encode_open_request(key, rows)),
                (serve.KIND_LP_ROUND, serve.encode_round_request(key, 1, serve.SESSION_SCORE, rnd)),
                (serve.KIND_LP_CLOSE, serve.encode_close_request(key, 1)),
                (serve.KIND_COLLECT, serve.encode_collect_request(key, snap, quality))]

    log = []
    with tempfile.TemporaryDirectory() as tmp:
        server = _server(tmp, log, ensembles={"ens": ["c", "a"]})
        try:
            conn = _FakeConn()
            server._buffers[conn] = bytearray()
            pending = []
            for kind, message in others("ens"):
                conn.inbox.append(_frame(message))
                server._read(conn, pending)
            # what an unknown model gets for a kind that names one
            conn.inbox.append(_frame(serve.encode_request("ent", serve.KIND_SCORE, state)))
            server._read(conn, pending)
            assert not pending and server.stats["errors"] == 6 and not log
            unknown = conn.sent[5].replace(b"ent", b"ens")
            for (kind, _), sent in zip(others("ens"), conn.sent):
                assert sent == unknown, kind
                with pytest.raises(serve.ServerError, match="no model 'ens'"):
                    serve.decode_reply(sent[4:])
            # kind 10 and the other unknown numbers stay unknown, under any name
            raw = bytearray(serve.encode_close_request("ens", 1))
            for number in (10, 12, 255):
                raw[4] = number
                with pytest.raises(serve.ProtocolError):
                    serve.decode_request(bytes(raw))
            # the request that follows a refused one is served
            conn.inbox.append(_frame(serve.encode_request("ens", serve.KIND_SCORE, state)))
            server._read(conn, pending)
            server._serve(pending)
            assert log == [("ensemble", "score_ensemble", ("c", "a"), False)] and len(conn.sent) == 7
            assert serve.decode_reply(conn.sent[6][4:])[0][0].tolist() == [7.0, 7.0]
        finally:
            server.close()
